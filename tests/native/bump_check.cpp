// bump_check.cpp — TEST INFRASTRUCTURE.  The bump and normal maps' host half
// (csrc/mcpt_host.cpp: mcpt_mtl_bump_maps_from_text, a parser of files from
// outside) under AddressSanitizer + UndefinedBehaviorSanitizer (built with
// -fsanitize=address,undefined and run by tests/test_bump_cpu.py, on the CPU).
// Every input lives in a heap block of exactly its length and every output in
// one of exactly the size the call may write, so a read or write past either
// is a sanitizer report.
//   bump_asan
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

struct Map {
  std::string name;
  int32_t kind;
  float bm;
};

// parse `text` from an exact-size heap copy: the count query, then exact-size outputs
int maps(const std::string &text, std::vector<Map> *out = nullptr) {
  std::unique_ptr<char[]> in(new char[text.size() ? text.size() : 1]);
  if (!text.empty()) std::memcpy(in.get(), text.data(), text.size());
  const int64_t n = (int64_t)text.size();
  int64_t nb = -1, nm = -1;
  int rc = mcpt_mtl_bump_maps_from_text(in.get(), n, nullptr, nullptr, nullptr, &nb, &nm);
  if (rc != MCPT_OK) return rc;
  std::unique_ptr<char[]> buf(new char[nb ? nb : 1]);
  std::unique_ptr<int32_t[]> kinds(new int32_t[nm ? nm : 1]);
  std::unique_ptr<float[]> bm(new float[nm ? nm : 1]);
  int64_t cap = nb, nm2 = nm;
  rc = mcpt_mtl_bump_maps_from_text(in.get(), n, buf.get(), kinds.get(), bm.get(), &cap, &nm2);
  expect(rc == MCPT_OK && cap == nb && nm2 == nm, "the second call agrees with the first");
  if (rc == MCPT_OK && out) {
    out->clear();
    const char *p = buf.get();
    for (int64_t i = 0; i < nm; ++i) {
      out->push_back(Map{std::string(p), kinds[i], bm[i]});
      p += out->back().name.size() + 1;
    }
    expect(p == buf.get() + nb, "the names fill the buffer exactly");
  }
  if (rc == MCPT_OK && nb > 0) {  // one byte short: refused, nothing written past the block
    std::unique_ptr<char[]> b1(new char[nb - 1 ? nb - 1 : 1]);
    int64_t small = nb - 1, m1 = nm;
    expect(mcpt_mtl_bump_maps_from_text(in.get(), n, b1.get(), kinds.get(), bm.get(), &small, &m1) == MCPT_ERR_ARG,
           "a short name buffer is refused");
  }
  if (rc == MCPT_OK && nm > 0) {  // one material short
    std::unique_ptr<int32_t[]> k1(new int32_t[nm - 1 ? nm - 1 : 1]);
    std::unique_ptr<float[]> f1(new float[nm - 1 ? nm - 1 : 1]);
    int64_t c2 = nb, m1 = nm - 1;
    expect(mcpt_mtl_bump_maps_from_text(in.get(), n, buf.get(), k1.get(), f1.get(), &c2, &m1) == MCPT_ERR_ARG,
           "short kinds and bm are refused");
  }
  return rc;
}

}  // namespace

int main() {
  std::vector<Map> m;
  expect(maps("", &m) == MCPT_OK && m.empty(), "empty text");
  expect(maps("map_Bump a.png\n", &m) == MCPT_OK && m.empty(), "a map before any newmtl is dropped");
  expect(maps("newmtl a\nmap_Bump a.png\nnewmtl b\nmap_bump b.png\nnewmtl c\nbump c.png\nnewmtl d\nnorm d.png\nnewmtl e\n", &m) ==
                 MCPT_OK &&
             m.size() == 5 && m[0].name == "a.png" && m[0].kind == MCPT_BUMP_HEIGHT && m[1].name == "b.png" &&
             m[1].kind == MCPT_BUMP_HEIGHT && m[2].name == "c.png" && m[2].kind == MCPT_BUMP_HEIGHT &&
             m[3].name == "d.png" && m[3].kind == MCPT_BUMP_NORMAL && m[4].name.empty() && m[4].kind == MCPT_BUMP_NONE &&
             m[0].bm == 1.0f && m[4].bm == 1.0f,
         "each keyword");
  expect(maps("newmtl a\nbump -bm 0.25 -s 2 2 a.png", &m) == MCPT_OK && m.size() == 1 && m[0].bm == 0.25f && m[0].name == "a.png",
         "-bm before other options, no newline at the end");
  expect(maps("newmtl a\nbump -clamp on -o 1 -bm 3 a b.png \r\n", &m) == MCPT_OK && m[0].bm == 3.0f && m[0].name == "a b.png",
         "-bm after other options");
  expect(maps("newmtl a\nnorm n.png\nbump -bm 2 h.png\n", &m) == MCPT_OK && m[0].name == "n.png" &&
             m[0].kind == MCPT_BUMP_NORMAL && m[0].bm == 1.0f,
         "norm wins over a later height map");
  expect(maps("newmtl a\nbump -bm 2 h.png\nnorm n.png\n", &m) == MCPT_OK && m[0].name == "n.png" &&
             m[0].kind == MCPT_BUMP_NORMAL && m[0].bm == 1.0f,
         "norm wins over an earlier height map");
  expect(maps("newmtl a\nbump tex\\sub\\h.png\n", &m) == MCPT_OK && m[0].name == "tex/sub/h.png", "backslashes");
  // truncated and malformed lines: options without a name, -bm without or with a bad value
  for (const char *t : {"newmtl a\nbump", "newmtl a\nbump ", "newmtl a\nbump -bm", "newmtl a\nbump -bm ", "newmtl a\nbump -bm 2",
                        "newmtl a\nbump -mm 1", "newmtl a\nbump -s 1 2 3", "newmtl a\nnorm -o", "newmtl a\nbump -bm x",
                        "newmtl", "\n\n\r\n", "bump\nnorm\nnewmtl\nbump -bm"}) {
    expect(maps(t, &m) == MCPT_OK, std::string("truncated: ") + t);
    for (const Map &x : m) expect(x.name.empty() && x.kind == MCPT_BUMP_NONE && x.bm == 1.0f, std::string("no map from: ") + t);
  }
  expect(maps("newmtl a\nbump -bm x h.png\n", &m) == MCPT_OK && m[0].name == "h.png" && m[0].bm == 1.0f,
         "an unusable -bm value keeps 1");
  expect(maps("newmtl a\nbump -bm 1e999 h.png\n", &m) == MCPT_OK && m[0].name == "h.png" && m[0].bm == 1.0f &&
             std::isfinite(m[0].bm),
         "an overflowing -bm value keeps 1");
  expect(maps("newmtl a\nbump -bm nan h.png\n", &m) == MCPT_OK && std::isfinite(m[0].bm), "a nan -bm value keeps 1");
  expect(maps("newmtl a\nbump -bm " + std::string(5000, '9') + " h.png\n", &m) == MCPT_OK && m[0].name == "h.png" &&
             std::isfinite(m[0].bm),
         "a 5000-digit -bm value");
  expect(maps("newmtl a\nbump " + std::string(70000, 'x') + ".png\n", &m) == MCPT_OK && m[0].name.size() == 70004, "a long name");
  {
    std::string many;
    for (int i = 0; i < 3000; ++i) many += "newmtl m\nbump -bm 2 a.png\nnorm b.png\n";
    expect(maps(many, &m) == MCPT_OK && m.size() == 3000 && m[2999].name == "b.png", "3000 materials");
  }
  int64_t nb = 0, nm = 0;
  expect(mcpt_mtl_bump_maps_from_text(nullptr, 5, nullptr, nullptr, nullptr, &nb, &nm) == MCPT_ERR_ARG, "null text with a length");
  expect(mcpt_mtl_bump_maps_from_text("x", -1, nullptr, nullptr, nullptr, &nb, &nm) == MCPT_ERR_ARG, "negative length");
  expect(mcpt_mtl_bump_maps_from_text("x", 1, nullptr, nullptr, nullptr, nullptr, &nm) == MCPT_ERR_ARG, "null n_bytes");
  char one[8];
  nb = 8, nm = 1;
  expect(mcpt_mtl_bump_maps_from_text("newmtl a\n", 9, one, nullptr, nullptr, &nb, &nm) == MCPT_ERR_ARG, "names without kinds");
  expect(mcpt_load_mtl_bump_maps("/nonexistent-directory/", "x.obj", nullptr, nullptr, nullptr, &nb, &nm) == MCPT_ERR_IO,
         "a missing OBJ file");
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
