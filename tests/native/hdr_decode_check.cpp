// hdr_decode_check.cpp — TEST INFRASTRUCTURE.  mcpt_decode_hdr (csrc/mcpt_host.cpp),
// a parser of files from outside, under AddressSanitizer + UndefinedBehaviorSanitizer
// (built with -fsanitize=address,undefined and run by tests/test_env_cpu.py, on the CPU):
// the committed stb goldens decode and re-encode to their own bytes, and every
// malformed case returns an error.  Every input lives in a heap block of exactly
// its length and every output in one of exactly width * height * 3 floats, so a
// read or write past either is a sanitizer report.
//   hdr_asan <repo root>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mcpt_hip.h"

namespace {

int failures = 0;

void expect(bool ok, const std::string &what) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s\n", what.c_str());
  }
}

std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// decode `n` bytes from an exact-size heap copy; on success *out holds the image
int decode(const uint8_t *src, size_t n, int32_t *w, int32_t *h, std::vector<float> *out = nullptr) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(in.get(), src, n);
  *w = *h = 0;
  int rc = mcpt_decode_hdr(in.get(), (int64_t)n, w, h, nullptr, 0);
  if (rc != MCPT_OK) return rc;
  const size_t floats = (size_t)*w * (size_t)*h * 3;
  std::unique_ptr<float[]> img(new float[floats]);
  rc = mcpt_decode_hdr(in.get(), (int64_t)n, w, h, img.get(), (int64_t)floats);
  if (rc == MCPT_OK && out) out->assign(img.get(), img.get() + floats);
  return rc;
}

std::vector<uint8_t> bytes_of(const std::string &s) { return std::vector<uint8_t>(s.begin(), s.end()); }

const char kHead[] = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n";

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s <repo root>\n", argv[0]);
    return 2;
  }
  const std::string golden = std::string(argv[1]) + "/tests/golden/";
  int32_t w = 0, h = 0;
  for (const char *name : {"stb_synthetic.hdr", "stb_narrow.hdr"}) {
    const std::vector<uint8_t> file = slurp(golden + name);
    expect(!file.empty(), std::string(name) + ": golden read");
    std::vector<float> rgb;
    expect(decode(file.data(), file.size(), &w, &h, &rgb) == MCPT_OK, std::string(name) + ": decodes");
    if (rgb.empty()) continue;
    // re-encode (rows already in file order: no flip) and compare with the file
    std::vector<float> rgba((size_t)w * h * 4, 0.0f);
    for (size_t i = 0; i < (size_t)w * h; ++i) std::memcpy(&rgba[4 * i], &rgb[3 * i], 12);
    const int64_t n = mcpt_encode_hdr(w, h, rgba.data(), 0, nullptr, 0);
    std::vector<uint8_t> again((size_t)(n > 0 ? n : 0));
    if (n > 0) mcpt_encode_hdr(w, h, rgba.data(), 0, again.data(), n);
    expect(again == file, std::string(name) + ": re-encoding reproduces the file");
    // a too-small output buffer is refused
    std::unique_ptr<float[]> small(new float[rgb.size() - 1]);
    expect(mcpt_decode_hdr(file.data(), (int64_t)file.size(), &w, &h, small.get(), (int64_t)rgb.size() - 1) == MCPT_ERR_ARG,
           std::string(name) + ": short output buffer");
    // truncations: every length of the narrow (flat) file, every 5th of the RLE one and its last 64
    const size_t step = file.size() > 4096 ? 5 : 1;
    for (size_t len = 0; len < file.size(); len += (len + 64 >= file.size() ? 1 : step))
      expect(decode(file.data(), len, &w, &h) < 0, std::string(name) + ": truncated at " + std::to_string(len));
  }
  // an RLE scanline of width 8: header, then four components
  auto rle = [&](const std::string &res, const std::vector<uint8_t> &body) {
    std::vector<uint8_t> f = bytes_of(std::string(kHead) + res);
    f.insert(f.end(), body.begin(), body.end());
    return f;
  };
  const std::vector<uint8_t> good_body = {2, 2, 0, 8, 0x88, 10, 0x88, 20, 0x88, 30, 8, 128, 128, 128, 128, 129, 129, 129, 129};
  {
    const std::vector<uint8_t> f = rle("-Y 1 +X 8\n", good_body);
    std::vector<float> rgb;
    expect(decode(f.data(), f.size(), &w, &h, &rgb) == MCPT_OK && w == 8 && h == 1, "hand-made RLE scanline decodes");
    expect(rgb.size() == 24 && rgb[0] == 10.0f / 256 && rgb[1] == 20.0f / 256 && rgb[23] == 30.0f / 128,
           "hand-made RLE scanline values (m * 2^(e - 136))");
  }
  struct Bad {
    const char *what;
    std::vector<uint8_t> file;
  };
  std::vector<uint8_t> long_run = good_body, long_raw = good_body, zero_run = good_body, wide = good_body;
  long_run[4] = 0x89;                    // a run of 9 in a scanline of 8
  long_raw[10] = 9;                      // 9 literal bytes where 8 remain
  zero_run[4] = 0x80;                    // a run of 0
  wide[3] = 9;                           // the scanline says 9 pixels, the header 8
  std::vector<uint8_t> second_run = good_body;
  second_run[4] = 0x84, second_run.insert(second_run.begin() + 6, {0x85, 11});  // 4 + 5 > 8
  const std::vector<Bad> bad = {
      {"run longer than the scanline", rle("-Y 1 +X 8\n", long_run)},
      {"second run past the scanline's end", rle("-Y 1 +X 8\n", second_run)},
      {"literal run longer than the scanline", rle("-Y 1 +X 8\n", long_raw)},
      {"run of zero length", rle("-Y 1 +X 8\n", zero_run)},
      {"scanline width disagrees with the header", rle("-Y 1 +X 8\n", wide)},
      {"second scanline is not RLE", rle("-Y 2 +X 8\n", [&] {
         std::vector<uint8_t> b = good_body;
         b.insert(b.end(), {1, 2, 3, 4});
         return b;
       }())},
      {"no magic", bytes_of("FORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\nabcd")},
      {"wrong magic", bytes_of("#?RADIANT\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\nabcd")},
      {"no FORMAT line", bytes_of("#?RADIANCE\n\n-Y 1 +X 1\nabcd")},
      {"other format", bytes_of("#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\nabcd")},
      {"+Y resolution", bytes_of(std::string(kHead) + "+Y 1 +X 1\nabcd")},
      {"X before Y", bytes_of(std::string(kHead) + "+X 1 -Y 1\nabcd")},
      {"zero width", bytes_of(std::string(kHead) + "-Y 1 +X 0\nabcd")},
      {"negative height", bytes_of(std::string(kHead) + "-Y -1 +X 1\nabcd")},
      {"no numbers", bytes_of(std::string(kHead) + "-Y  +X \nabcd")},
      {"trailing text in the resolution", bytes_of(std::string(kHead) + "-Y 1 +X 1 junk\nabcd")},
      {"huge number", bytes_of(std::string(kHead) + "-Y 99999999999999999999999 +X 1\nabcd")},
      {"product beyond 2^26", bytes_of(std::string(kHead) + "-Y 8193 +X 8192\nabcd")},
      {"product overflowing int32", bytes_of(std::string(kHead) + "-Y 2147483647 +X 2147483647\nabcd")},
      {"header without its empty line", bytes_of("#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n-Y 1 +X 1\nabcd")},
      {"header line without newline", bytes_of("#?RADIANCE")},
      {"a 2000-character header line", bytes_of("#?RADIANCE\n" + std::string(2000, 'x') + "\n\n-Y 1 +X 1\nabcd")},
      {"empty", {}},
  };
  for (const Bad &b : bad) expect(decode(b.file.data(), b.file.size(), &w, &h) < 0, b.what);
  // the largest product allowed passes the header (the size query reads no pixel)
  {
    const std::vector<uint8_t> f = bytes_of(std::string(kHead) + "-Y 8192 +X 8192\n");
    expect(mcpt_decode_hdr(f.data(), (int64_t)f.size(), &w, &h, nullptr, 0) == MCPT_OK && w == 8192 && h == 8192,
           "2^26 texels is within the limit");
  }
  // a flat file of a wide-enough image (stb's turn at the first scanline)
  {
    std::vector<uint8_t> f = bytes_of(std::string(kHead) + "-Y 1 +X 8\n");
    for (int i = 0; i < 8; ++i) f.insert(f.end(), {(uint8_t)(i + 1), 0, 0, 136});
    std::vector<float> rgb;
    expect(decode(f.data(), f.size(), &w, &h, &rgb) == MCPT_OK && rgb.size() == 24 && rgb[0] == 1.0f && rgb[21] == 8.0f,
           "flat scanlines of a width-8 image");
    expect(decode(f.data(), f.size() - 1, &w, &h) < 0, "flat scanlines truncated");
  }
  expect(mcpt_decode_hdr(nullptr, 0, &w, &h, nullptr, 0) == MCPT_ERR_ARG, "null input");
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
