// smooth_check.cpp — TEST INFRASTRUCTURE.  Smooth shading's host half
// (csrc/mcpt_host.cpp: mcpt_vertex_normals, which indexes a mesh from outside,
// and mcpt_obj_normals_from_text, a parser of files from outside) under
// AddressSanitizer + UndefinedBehaviorSanitizer (built with
// -fsanitize=address,undefined and run by tests/test_smooth_cpu.py, on the
// CPU).  Every input lives in a heap block of exactly its length and every
// output in one of exactly the size the call may write, so a read or write past
// either is a sanitizer report.
//   smooth_asan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
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

// parse `text` from an exact-size heap copy: the count query, then exact-size outputs
int parse(const std::string &text, std::vector<float> *vn = nullptr, std::vector<uint8_t> *has = nullptr) {
  const size_t n = text.size();
  std::unique_ptr<char[]> in(new char[n ? n : 1]);
  if (n) std::memcpy(in.get(), text.data(), n);
  int64_t nt = 0;
  int rc = mcpt_obj_normals_from_text(in.get(), (int64_t)n, nullptr, nullptr, &nt);
  if (rc != MCPT_OK) return rc;
  std::unique_ptr<float[]> v(new float[nt ? 9 * nt : 1]);
  std::unique_ptr<uint8_t[]> h(new uint8_t[nt ? nt : 1]);
  int64_t cap = nt;
  rc = mcpt_obj_normals_from_text(in.get(), (int64_t)n, v.get(), h.get(), &cap);
  if (rc == MCPT_OK && vn) vn->assign(v.get(), v.get() + 9 * nt);
  if (rc == MCPT_OK && has) has->assign(h.get(), h.get() + nt);
  if (rc == MCPT_OK && nt > 0) {  // one triangle short: refused, nothing written past the block
    std::unique_ptr<float[]> v1(new float[9 * (nt - 1) + 1]);
    std::unique_ptr<uint8_t[]> h1(new uint8_t[nt]);
    int64_t small = nt - 1;
    expect(mcpt_obj_normals_from_text(in.get(), (int64_t)n, v1.get(), h1.get(), &small) == MCPT_ERR_ARG,
           "short output buffers are refused");
  }
  return rc;
}

// triangles -> packed records in an exact-size block, normals by the caller
struct Mesh {
  std::unique_ptr<mcpt_triangle[]> t;
  int64_t n;
};
Mesh mesh(const std::vector<float> &verts /* n x 9 */) {
  Mesh m;
  m.n = (int64_t)(verts.size() / 9);
  m.t.reset(new mcpt_triangle[m.n ? m.n : 1]);
  std::unique_ptr<int32_t[]> idx(new int32_t[m.n ? m.n : 1]);
  for (int64_t i = 0; i < m.n; ++i) {
    std::memset(&m.t[i], 0, sizeof(mcpt_triangle));
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) m.t[i].v[k][c] = verts[9 * i + 3 * k + c];
    idx[i] = 0;
  }
  expect(mcpt_pack_triangles(m.t.get(), idx.get(), m.n) == MCPT_OK, "pack_triangles");
  return m;
}
int generate(const Mesh &m, double crease, std::vector<float> *out = nullptr) {
  std::unique_ptr<float[]> vn(new float[m.n ? 9 * m.n : 1]);
  const int rc = mcpt_vertex_normals(m.t.get(), m.n, crease, vn.get());
  if (rc == MCPT_OK && out) out->assign(vn.get(), vn.get() + 9 * m.n);
  return rc;
}

const char kGood[] =
    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 2\nvn 0 1 0\n"
    "f 1//1 2//1 3//1\nf 1/1/1 2/1/2 3/1/-1 4/1/-2\nf 1 2 3\n";

}  // namespace

int main() {
  // ---- the parser
  {
    std::vector<float> vn;
    std::vector<uint8_t> has;
    expect(parse(kGood, &vn, &has) == MCPT_OK && has.size() == 4, "good file parses into 4 triangles");
    if (has.size() == 4) {
      expect(has[0] == 1 && has[1] == 1 && has[2] == 1 && has[3] == 0, "has flags");
      expect(vn[2] == 1.0f && vn[0] == 0.0f, "vn normalised");
      expect(vn[9 + 3 + 1] == 1.0f && vn[9 + 6 + 1] == 1.0f, "second index and negative index");
    }
    // every truncation of the good file parses or fails cleanly
    const std::string g(kGood);
    for (size_t len = 0; len <= g.size(); ++len) {
      const int rc = parse(g.substr(0, len));
      expect(rc == MCPT_OK || rc == MCPT_ERR_PARSE, "truncated at " + std::to_string(len));
    }
  }
  struct Case {
    const char *what;
    std::string text;
    int rc;
  };
  const std::string head = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\n";
  const std::vector<Case> cases = {
      {"empty", "", MCPT_OK},
      {"no newline at the end", head + "f 1//1 2//1 3//1", MCPT_OK},
      {"vn index past the records", head + "f 1//2 2//1 3//1\n", MCPT_ERR_PARSE},
      {"vn index before the first", head + "f 1//-2 2//1 3//1\n", MCPT_ERR_PARSE},
      {"huge vn index", head + "f 1//99999999999999999999 2//1 3//1\n", MCPT_ERR_PARSE},
      {"huge negative vn index", head + "f 1//-99999999999999999999 2//1 3//1\n", MCPT_ERR_PARSE},
      {"face index 0", head + "f 0//1 2//1 3//1\n", MCPT_ERR_PARSE},
      {"vn defined after its use", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\nvn 0 0 1\n", MCPT_OK},
      {"slashes only", head + "f / // ///\n", MCPT_ERR_PARSE},
      {"trailing slash", head + "f 1/ 2// 3//1\n", MCPT_OK},
      {"letters for the normal", head + "f 1//x 2//y 3//z\n", MCPT_OK},
      {"a 100-character index", head + "f 1//" + std::string(100, '1') + " 2//1 3//1\n", MCPT_OK},
      {"vn with one number", "vn 1\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n", MCPT_OK},
      {"vn with no number", "vn\nvn \nv 0 0 0\nf 1//1 1//1 1//1\n", MCPT_OK},
      {"vn nan inf", "vn nan inf 1e999\nv 0 0 0\nf 1//1 1//1 1//1\n", MCPT_OK},
      {"face with two corners", head + "f 1//1 2//1\n", MCPT_OK},
      {"carriage returns", "v 0 0 0\r\nvn 0 0 1\r\nf 1//1 1//1 1//1\r\n", MCPT_OK},
      {"tabs", "v\t0 0 0\nvn\t0\t0\t1\nf\t1//1\t1//1\t1//1\n", MCPT_OK},
      {"binary noise", std::string("f \x01\x02//\xff\xfe \x00 1//1\n", 17), MCPT_ERR_PARSE},
      {"a lone f", "f", MCPT_OK},
      {"a lone vn", "vn", MCPT_OK},
  };
  for (const Case &c : cases) expect(parse(c.text) == c.rc, c.what);
  {
    int64_t nt = 0;
    expect(mcpt_obj_normals_from_text(nullptr, 0, nullptr, nullptr, &nt) == MCPT_OK && nt == 0, "null text of length 0");
    expect(mcpt_obj_normals_from_text(nullptr, 5, nullptr, nullptr, &nt) == MCPT_ERR_ARG, "null text of length 5");
    expect(mcpt_obj_normals_from_text("f", -1, nullptr, nullptr, &nt) == MCPT_ERR_ARG, "negative length");
    expect(mcpt_obj_normals_from_text("f", 1, nullptr, nullptr, nullptr) == MCPT_ERR_ARG, "null count");
    float one[9];
    nt = 1;
    expect(mcpt_obj_normals_from_text("f", 1, one, nullptr, &nt) == MCPT_ERR_ARG, "vn without has");
    expect(mcpt_load_obj_normals("/nonexistent/", "x.obj", nullptr, nullptr, &nt) == MCPT_ERR_IO, "missing file");
  }
  // ---- the generator
  {
    expect(mcpt_vertex_normals(nullptr, 0, 40.0, nullptr) == MCPT_OK, "empty mesh");
    expect(mcpt_vertex_normals(nullptr, 1, 40.0, nullptr) == MCPT_ERR_ARG, "null mesh of one triangle");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // a fold, a zero-area triangle, a point triangle, NaN and infinite corners, a twin with -0
    const Mesh m = mesh({0, 0, 0, 1, 0, 0, 0, 1, 0,          //
                         0, 0, 0, 0, 1, 0, -1, 0, 0.5f,      //
                         0, 0, 0, 0, 0, 1, 0, 0, 2,          //
                         1, 1, 1, 1, 1, 1, 1, 1, 1,          //
                         nan, 0, 0, 1, 0, 0, 0, 1, 0,        //
                         inf, 0, 0, 1, 0, 0, 0, 1, 0,        //
                         -0.0f, -0.0f, -0.0f, 1, 0, 0, 0, 1, 0});
    std::vector<float> vn;
    expect(generate(m, 40.0, &vn) == MCPT_OK && vn.size() == 63, "mixed mesh");
    for (int i : {2, 3, 4, 5})  // degenerate triangles keep their own (non-finite) normal's bits
      expect(!vn.empty() && std::memcmp(&vn[9 * i], m.t[i].normal, 12) == 0, "degenerate triangle " + std::to_string(i));
    expect(!vn.empty() && std::memcmp(&vn[0], &vn[9 * 6], 36) == 0, "the -0 twin welds to the same normals");
    expect(!vn.empty() && std::memcmp(&vn[0], m.t[0].normal, 12) != 0, "the fold is smoothed at the shared vertex");
    for (double bad : {-1.0, 181.0, (double)nan}) expect(generate(m, bad) == MCPT_ERR_ARG, "crease out of range");
    expect(generate(m, 0.0, &vn) == MCPT_OK, "crease 0");
    for (int i : {0, 1, 6})
      for (int k = 0; k < 3; ++k)
        expect(std::memcmp(&vn[9 * i + 3 * k], m.t[i].normal, 12) == 0, "crease 0 is flat");
    expect(generate(m, 180.0) == MCPT_OK, "crease 180");
    // a fan of 500 triangles around one apex (one welded vertex of 500 corners)
    std::vector<float> fan;
    for (int i = 0; i < 500; ++i) {
      const float a = 6.2831853f * i / 500, b = 6.2831853f * (i + 1) / 500;
      const float tri[9] = {0, 0, 1, std::cos(a), std::sin(a), 0, std::cos(b), std::sin(b), 0};
      fan.insert(fan.end(), tri, tri + 9);
    }
    expect(generate(mesh(fan), 180.0, &vn) == MCPT_OK, "fan");  // (180: every face joins)
    expect(std::fabs(vn[2] - 1.0f) < 1e-5f && std::fabs(vn[0]) < 1e-5f, "the apex normal of a symmetric fan is the axis");
    // the same fan as a shallow cap (one narrow cone of normals: the linear path) and as a spire of
    // 65,537 corners (the pairwise path's limit)
    auto cap = [](int m, float slope) {
      std::vector<float> f;
      for (int i = 0; i < m; ++i) {
        const float a = 6.2831853f * i / m, b = 6.2831853f * (i + 1) / m;
        const float tri[9] = {0, 0, 1, std::cos(a), std::sin(a), 1 - slope, std::cos(b), std::sin(b), 1 - slope};
        f.insert(f.end(), tri, tri + 9);
      }
      return f;
    };
    expect(generate(mesh(cap(70000, 0.02f)), 40.0, &vn) == MCPT_OK, "a pole of 70,000 corners");
    expect(std::fabs(vn[2] - 1.0f) < 1e-5f && std::memcmp(&vn[0], &vn[9 * 69999], 12) == 0, "the pole has one normal");
    expect(generate(mesh(cap(65537, 1.0f)), 40.0) == MCPT_ERR_LIMIT, "a spire of 65,537 corners is refused");
    expect(generate(mesh(cap(2000, 1.0f)), 40.0, &vn) == MCPT_OK, "a spire of 2,000 corners");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
