// cutout_check.cpp — TEST INFRASTRUCTURE.  The cutouts' host half
// (csrc/mcpt_host.cpp: mcpt_mtl_alpha_maps_from_text, the `map_d` parser of
// files from outside) under AddressSanitizer + UndefinedBehaviorSanitizer
// (built with -fsanitize=address,undefined and run by tests/test_cutout_cpu.py,
// on the CPU).  Every input lives in a heap block of exactly its length and
// every output in one of exactly the size the call may write, so a read or
// write past either is a sanitizer report.
//   cutout_asan
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

typedef int (*MapsFn)(const char *, int64_t, char *, int64_t *, int64_t *);

// parse `text` from an exact-size heap copy: the count query, then an exact-size name buffer
int maps(MapsFn fn, const std::string &text, std::vector<std::string> *names = nullptr) {
  const auto in = exact(text);
  const int64_t n = (int64_t)text.size();
  int64_t nb = -1, nm = -1;
  int rc = fn(in.get(), n, nullptr, &nb, &nm);
  if (rc != MCPT_OK) return rc;
  std::unique_ptr<char[]> buf(new char[nb ? nb : 1]);
  int64_t cap = nb, nm2 = -1;
  rc = fn(in.get(), n, buf.get(), &cap, &nm2);
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
    expect(fn(in.get(), n, b1.get(), &small, &m) == MCPT_ERR_ARG, "a short name buffer is refused");
  }
  return rc;
}

int alpha(const std::string &text, std::vector<std::string> *names = nullptr) {
  return maps(mcpt_mtl_alpha_maps_from_text, text, names);
}

}  // namespace

int main() {
  std::vector<std::string> names, kd;
  expect(alpha("newmtl leaf\nKd 1 1 1\nmap_Kd leaf.png\nmap_d leaf_mask.png\nnewmtl bark\nmap_Kd bark.png\nnewmtl fence\n"
               "map_d  dir\\sub dir\\m x.png \r\n",
               &names) == MCPT_OK &&
             names.size() == 3 && names[0] == "leaf_mask.png" && names[1].empty() && names[2] == "dir/sub dir/m x.png",
         "names, none, spaces and backslashes");
  // map_d and map_Kd are told apart, and neither reader sees the other's names
  expect(maps(mcpt_mtl_maps_from_text, "newmtl leaf\nmap_d mask.png\nmap_Kd leaf.png\nnewmtl b\nmap_d only.png\n", &kd) == MCPT_OK &&
             kd.size() == 2 && kd[0] == "leaf.png" && kd[1].empty(),
         "map_Kd's reader skips map_d");
  expect(alpha("newmtl a\nmap_Kd colour.png\nd 0.5\nTr 0.5\nmap_D upper.png\nmap_dx no.png\n", &names) == MCPT_OK && names.size() == 1 &&
             names[0].empty(),
         "map_Kd, the d and Tr scalars and other spellings are no map_d");
  expect(alpha("newmtl a\nmap_d -s 1 2 3 -o 0.5 -clamp on -imfchan m -mm 0 1 -blendu off mask.png\n", &names) == MCPT_OK &&
             names.size() == 1 && names[0] == "mask.png",
         "options are skipped");
  for (const char *line : {"map_d", "map_d ", "map_d -clamp on", "map_d -s 1 1 1", "map_d -mm 0", "map_d -o", "map_d -imfchan"})
    expect(alpha(std::string("newmtl a\n") + line, &names) == MCPT_OK && names.size() == 1 && names[0].empty(),
           std::string("option-only line: ") + line);
  expect(alpha("map_d early.png\nnewmtl a\n", &names) == MCPT_OK && names.size() == 1 && names[0].empty(), "a map before any material");
  expect(alpha("newmtl a\nmap_d one.png\nmap_d two.png\nnewmtl a\n", &names) == MCPT_OK && names.size() == 2 && names[0] == "two.png" &&
             names[1].empty(),
         "the last map of a material; a repeated name is another record");
  expect(alpha("", &names) == MCPT_OK && names.empty() && alpha("\n", &names) == MCPT_OK && alpha("newmtl", &names) == MCPT_OK &&
             names.size() == 1,
         "empty inputs");
  {
    // truncated text: every prefix parses, never read past
    const std::string full = "newmtl a\nmap_Kd c.png\nmap_d -s 1 1 1 -o 0 0 a\\b c.png\nnewmtl b\nmap_d -clamp on";
    for (size_t n = 0; n <= full.size(); ++n) expect(alpha(full.substr(0, n)) == MCPT_OK, "mtl prefix " + std::to_string(n));
    int64_t nb = 0, nm = 0;
    expect(mcpt_mtl_alpha_maps_from_text(nullptr, 0, nullptr, &nb, &nm) == MCPT_OK && nb == 0 && nm == 0, "null text of length 0");
    expect(mcpt_mtl_alpha_maps_from_text(nullptr, 3, nullptr, &nb, &nm) == MCPT_ERR_ARG, "null mtl text");
    expect(mcpt_mtl_alpha_maps_from_text("x", -1, nullptr, &nb, &nm) == MCPT_ERR_ARG, "negative length");
    expect(mcpt_mtl_alpha_maps_from_text("x", 1, nullptr, nullptr, &nm) == MCPT_ERR_ARG, "null byte count");
    expect(mcpt_mtl_alpha_maps_from_text("x", 1, nullptr, &nb, nullptr) == MCPT_ERR_ARG, "null material count");
    expect(mcpt_load_mtl_alpha_maps(nullptr, "a.obj", nullptr, &nb, &nm) == MCPT_ERR_ARG, "null directory");
    expect(mcpt_load_mtl_alpha_maps("/nonexistent-directory/", "a.obj", nullptr, &nb, &nm) == MCPT_ERR_IO, "a missing OBJ file");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
