// texture_check.cpp — TEST INFRASTRUCTURE.  The texture maps' host half
// (csrc/mcpt_host.cpp: mcpt_obj_uvs_from_text and mcpt_mtl_maps_from_text,
// parsers of files from outside) under AddressSanitizer +
// UndefinedBehaviorSanitizer (built with -fsanitize=address,undefined and run
// by tests/test_texture_cpu.py, on the CPU).  Every input lives in a heap
// block of exactly its length and every output in one of exactly the size the
// call may write, so a read or write past either is a sanitizer report.
//   texture_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

std::unique_ptr<char[]> exact(const std::string &text) {
  std::unique_ptr<char[]> in(new char[text.size() ? text.size() : 1]);
  if (!text.empty()) std::memcpy(in.get(), text.data(), text.size());
  return in;
}

// parse `text` from an exact-size heap copy: the count query, then exact-size outputs
int uvs(const std::string &text, std::vector<float> *uv = nullptr, std::vector<uint8_t> *has = nullptr) {
  const auto in = exact(text);
  const int64_t n = (int64_t)text.size();
  int64_t nt = 0;
  int rc = mcpt_obj_uvs_from_text(in.get(), n, nullptr, nullptr, &nt);
  if (rc != MCPT_OK) return rc;
  std::unique_ptr<float[]> v(new float[nt ? 6 * nt : 1]);
  std::unique_ptr<uint8_t[]> h(new uint8_t[nt ? nt : 1]);
  int64_t cap = nt;
  rc = mcpt_obj_uvs_from_text(in.get(), n, v.get(), h.get(), &cap);
  if (rc == MCPT_OK && uv) uv->assign(v.get(), v.get() + 6 * nt);
  if (rc == MCPT_OK && has) has->assign(h.get(), h.get() + nt);
  if (rc == MCPT_OK && nt > 0) {  // one triangle short: refused, nothing written past the block
    std::unique_ptr<float[]> v1(new float[6 * (nt - 1) + 1]);
    std::unique_ptr<uint8_t[]> h1(new uint8_t[nt]);
    int64_t small = nt - 1;
    expect(mcpt_obj_uvs_from_text(in.get(), n, v1.get(), h1.get(), &small) == MCPT_ERR_ARG, "short uv buffers are refused");
  }
  return rc;
}

int maps(const std::string &text, std::vector<std::string> *names = nullptr) {
  const auto in = exact(text);
  const int64_t n = (int64_t)text.size();
  int64_t nb = -1, nm = -1;
  int rc = mcpt_mtl_maps_from_text(in.get(), n, nullptr, &nb, &nm);
  if (rc != MCPT_OK) return rc;
  std::unique_ptr<char[]> buf(new char[nb ? nb : 1]);
  int64_t cap = nb, nm2 = -1;
  rc = mcpt_mtl_maps_from_text(in.get(), n, buf.get(), &cap, &nm2);
  expect(rc == MCPT_OK && cap == nb && nm2 == nm, "the second call agrees with the first");
  if (rc == MCPT_OK && names) {
    names->clear();
    const char *p = buf.get();
    for (int64_t k = 0; k < nm; ++k) {
      names->push_back(std::string(p));
      p += names->back().size() + 1;
    }
    expect(p == buf.get() + nb, "the names fill the buffer exactly");
  }
  if (rc == MCPT_OK && nb > 0) {
    std::unique_ptr<char[]> b1(new char[nb - 1 ? nb - 1 : 1]);
    int64_t small = nb - 1, m = 0;
    expect(mcpt_mtl_maps_from_text(in.get(), n, b1.get(), &small, &m) == MCPT_ERR_ARG, "a short name buffer is refused");
  }
  return rc;
}

const char *kQuad =
    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"
    "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\n";

}  // namespace

int main() {
  std::vector<float> uv;
  std::vector<uint8_t> has;
  // the forms, a fan, negative indices
  expect(uvs(std::string(kQuad) + "f 1/1 2/2 3/3 4/4\n", &uv, &has) == MCPT_OK && has.size() == 2 && has[0] && has[1] &&
             uv[0] == 0 && uv[2] == 1 && uv[5] == 1 && uv[6] == 0 && uv[8] == 1 && uv[10] == 0 && uv[11] == 1,
         "v/vt fan");
  expect(uvs(std::string(kQuad) + "f 1/1/1 2/2/1 3/3/1\nf 1//1 2//1 3//1\nf 1 2 3\n", &uv, &has) == MCPT_OK &&
             has.size() == 3 && has[0] && !has[1] && !has[2] && uv[6] == 0 && uv[11] == 0,
         "v/vt/vn, v//vn, v");
  expect(uvs(std::string(kQuad) + "f -4/-4 -3/-3 -2/-2\n", &uv, &has) == MCPT_OK && has[0] && uv[2] == 1 && uv[4] == 1,
         "negative indices");
  expect(uvs(std::string(kQuad) + "f 1/1 2/2 3\n", &uv, &has) == MCPT_OK && !has[0] && uv[2] == 0, "a corner without vt");
  // out of range, zero, overflow, junk
  for (const char *face : {"f 1/5 2/2 3/3", "f 1/-5 2/2 3/3", "f 1/0 2/2 3/3", "f 1/99999999999999999999 2/2 3/3",
                           "f 1/-99999999999999999999 2/2 3/3", "f 1/123456789012345678901234567890 2/2 3/3", "f 1/x 2/2 3/3",
                           "f 1/1x 2/2 3/3", "f 0/1 2/2 3/3", "f x 2 3"})
    expect(uvs(std::string(kQuad) + face + "\n") == MCPT_ERR_PARSE, std::string("refused: ") + face);
  // a vt named before it is defined counts the records read so far
  expect(uvs("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/2 3/1\nvt 1 1\n") == MCPT_ERR_PARSE, "vt index past the records so far");
  // non-finite and short vt records
  expect(uvs("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt nan 0\nvt 0.5\nvt \nf 1/1 2/2 3/2\nf 1/2 2/2 3/2\nf 1/3 2/3 3/3\n", &uv, &has) == MCPT_OK &&
             has.size() == 3 && !has[0] && has[1] && uv[6] == 0.5f && uv[7] == 0 && !has[2],
         "nan, one-number and empty vt records");
  expect(uvs("vt 1e999 0\nv 0 0 0\nf 1/1 1/1 1/1\n", &uv, &has) == MCPT_OK && !has[0], "an overflowing coordinate is no vt");
  // truncated text: every prefix of a file parses or is refused, never read past
  {
    const std::string full = std::string(kQuad) + "f 1/1/1 2/2/1 3/3/1 4/4/1\nf -1/-1 -2/-2 -3/-3";
    for (size_t n = 0; n <= full.size(); ++n) {
      const int rc = uvs(full.substr(0, n));
      expect(rc == MCPT_OK || rc == MCPT_ERR_PARSE, "prefix " + std::to_string(n));
    }
  }
  expect(uvs("") == MCPT_OK && uvs("\n\n") == MCPT_OK && uvs("f") == MCPT_OK && uvs("vt") == MCPT_OK && uvs("f 1/") == MCPT_OK,
         "empty inputs");
  {
    int64_t nt = 0;
    expect(mcpt_obj_uvs_from_text(nullptr, 0, nullptr, nullptr, &nt) == MCPT_OK && nt == 0, "null text of length 0");
    expect(mcpt_obj_uvs_from_text(nullptr, 4, nullptr, nullptr, &nt) == MCPT_ERR_ARG, "null text of length 4");
    expect(mcpt_obj_uvs_from_text("f", -1, nullptr, nullptr, &nt) == MCPT_ERR_ARG, "negative length");
    float one[6];
    expect(mcpt_obj_uvs_from_text("f", 1, one, nullptr, &nt) == MCPT_ERR_ARG, "uv without has");
  }

  // map_Kd
  std::vector<std::string> names;
  expect(maps("newmtl a\nKd 1 1 1\nmap_Kd wood.png\nnewmtl b\nKd 0 0 0\nnewmtl c\nmap_Kd  dir\\sub dir\\t x.png \r\n", &names) == MCPT_OK &&
             names.size() == 3 && names[0] == "wood.png" && names[1].empty() && names[2] == "dir/sub dir/t x.png",
         "names, none, spaces and backslashes");
  expect(maps("newmtl a\nmap_Kd -s 1 2 3 -o 0.5 -clamp on -bm 0.2 -mm 0 1 -blendu off tex.png\n", &names) == MCPT_OK &&
             names.size() == 1 && names[0] == "tex.png",
         "options are skipped");
  expect(maps("newmtl a\nmap_Kd -s 2 2 1.png\n", &names) == MCPT_OK && names[0] == "1.png", "-s with two numbers before a numeric name");
  for (const char *line : {"map_Kd", "map_Kd ", "map_Kd -clamp on", "map_Kd -s 1 1 1", "map_Kd -mm 0", "map_Kd -o", "map_Kd -clamp"})
    expect(maps(std::string("newmtl a\n") + line, &names) == MCPT_OK && names.size() == 1 && names[0].empty(),
           std::string("option-only line: ") + line);
  expect(maps("map_Kd early.png\nnewmtl a\n", &names) == MCPT_OK && names.size() == 1 && names[0].empty(), "a map before any material");
  expect(maps("newmtl a\nmap_Kd one.png\nmap_Kd two.png\nnewmtl a\n", &names) == MCPT_OK && names.size() == 2 && names[0] == "two.png" &&
             names[1].empty(),
         "the last map of a material; a repeated name is another record");
  expect(maps("", &names) == MCPT_OK && names.empty() && maps("\n", &names) == MCPT_OK && maps("newmtl", &names) == MCPT_OK &&
             names.size() == 1,
         "empty inputs");
  {
    const std::string full = "newmtl a\nmap_Kd -s 1 1 1 -o 0 0 a\\b c.png\nnewmtl b\nmap_Kd -clamp on";
    for (size_t n = 0; n <= full.size(); ++n) expect(maps(full.substr(0, n)) == MCPT_OK, "mtl prefix " + std::to_string(n));
    int64_t nb = 0, nm = 0;
    expect(mcpt_mtl_maps_from_text(nullptr, 3, nullptr, &nb, &nm) == MCPT_ERR_ARG, "null mtl text");
    expect(mcpt_mtl_maps_from_text("x", 1, nullptr, nullptr, &nm) == MCPT_ERR_ARG, "null byte count");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
