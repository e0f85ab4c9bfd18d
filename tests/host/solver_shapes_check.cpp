// Stand-alone check of csrc/solver_shapes.h (host only; build with -fsanitize=address,undefined and run on its own):
//   solver_shapes_check tests/golden/broyden_schedule.json
// The table holds, per case, the inputs of a Broyden handle (sizes and environment knobs), the bytes the built library allocated
// for it and the launches of its update chain in a solve of `thr` iterations, recorded on the GPU (scripts/record_broyden_schedule.py).
// For every row this program derives the shape with broyden_shape, runs update_chain for k = 0 .. thr - 1 on a target that only
// records (pass name, stated bytes), and prints {"case", "nbytes", "iters"} in the table's form; the pytest test compares the two
// in both directions.  Independently of the table it asserts for every case
//   * k - keep0 + 1 <= PARTA_LD whenever a fold pass is issued (its kept pairs fit a row of partials; the register form's KB holds
//     them; the LDS form's dynamic LDS is 16 B x 256 threads per kept pair),
//   * u2d_kmax <= (u2d_reg ? U2R_KB_MAX : U2D_LDS_KMAX), also after the cap of a refused LDS attribute,
// and once: a request of 38 / 36 in the LDS form yields the shape of 31 / 31.
#include "solver_shapes.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

using shapes::BroydenShape;
using shapes::Knobs;
static int g_bad = 0;
static std::string g_case;

static void fail(const char* what, long long a = 0, long long b = 0) {
  printf("FAIL %s: %s (%lld, %lld)\n", g_case.c_str(), what, a, b);
  ++g_bad;
}

// The launches of one solver, under the names SingleTarget (solver.hip) reports them; groups / combine_due are its rules.
struct Recorder {
  BroydenShape sh;
  int64_t M = 0;
  int hist = 0;
  int ready = 0, from = 0;
  int64_t pending = 0;
  std::vector<std::pair<std::string, int64_t>> log;

  const BroydenShape& size_class() const { return sh; }
  void bytes(int64_t b) { pending = b; }
  int64_t vec_bytes() const { return M * 4; }
  int pair_elem_bytes() const { return hist ? 2 : 4; }
  int& a_ready() { return ready; }
  int& a_from() { return from; }
  int groups(int k) const { return (sh.jgroups > 1 && k >= 4 * sh.jgroups) ? sh.jgroups : 1; }
  bool combine_due(int, int G) const { return G > 1; }

  void pass(const char* name) {   // a launch takes the bytes stated for it; an unstated launch has none
    log.push_back({name, pending});
    pending = 0;
  }
  void sweep(const char* name) { pass((std::string(name) + (hist ? "_bf16" : "")).c_str()); }
  void fold(int k, int keep0, int room) {
    const int nk = k - keep0;
    if (keep0 < 0 || nk + 1 > PARTA_LD) fail("the fold's kept pairs do not fit a row of partials", k, keep0);
    if (nk > room) fail("the fold keeps more pairs than its form holds", nk, room);
    if (hist) fail("a bf16-history solver has no folded sweep");
    pass("k_sweep_u2d");
  }
  void sweep_u1(int) { sweep("k_sweep_u1"); }
  void reduce_a_check(int, double, int) { pass("k_reduce_check"); }
  void sweep_v(int) { sweep("k_sweep_v"); }
  void reduce_cb(int) { pass("k_reduce_cb"); }
  template <int KB>
  void sweep_u2r(int k, int keep0) {
    static_assert(KB <= U2R_KB_MAX, "register fold");
    fold(k, keep0, KB);
  }
  void sweep_u2d(int k, int keep0, size_t lds) {
    if (lds != (size_t)std::max(k - keep0, 1) * shapes::THREADS * 16 || lds > (size_t)U2D_LDS_KMAX * shapes::THREADS * 16)
      fail("dynamic LDS of the fold", k, (long long)lds);
    fold(k, keep0, U2D_LDS_KMAX);
  }
  void sweep_u2(int) { sweep("k_sweep_u2"); }
  void dots(int, int) { pass("k_dots"); }
  void reduce_check(int, double) { pass("k_reduce_check"); }
  void axpy(int, int, bool) { pass("k_axpy"); }
  void combine(int, int) { pass("k_axpy_combine"); }
  void final_pass(int, bool) { pass("k_final"); }
};

static void check_limits(const BroydenShape& s) {
  if (s.u2d_kmax > (s.u2d_reg ? U2R_KB_MAX : U2D_LDS_KMAX) || s.u2d_keep > s.u2d_kmax) fail("fold limits", s.u2d_kmax, s.u2d_keep);
}

// one solve of thr iterations; prints the row and returns the launches of all iterations
static std::vector<std::pair<std::string, int64_t>> run(const BroydenShape& sh, int64_t M, int hist, bool print) {
  check_limits(sh);
  Recorder t;
  t.sh = sh;
  t.M = M;
  t.hist = hist;
  std::vector<std::pair<std::string, int64_t>> all;
  if (print) printf("{\"case\": \"%s\", \"nbytes\": %zu, \"iters\": [", g_case.c_str(), sh.bytes.total());
  for (int k = 0; k < sh.thr; ++k) {
    t.log.clear();
    shapes::update_chain(t, k, 0.0);
    if (print) printf("%s[", k ? ", " : "");
    for (size_t i = 0; i < t.log.size(); ++i) {
      const int64_t b = t.log[i].second;
      if (b % M) fail("stated bytes are not a multiple of M", k, b);
      if (print) printf("%s[\"%s\", %lld]", i ? ", " : "", t.log[i].first.c_str(), (long long)(b / M));
      all.push_back(t.log[i]);
    }
    if (print) printf("]");
  }
  if (print) printf("]}\n");
  return all;
}

static bool same_shape(const BroydenShape& a, const BroydenShape& b) {
  return a.same_size_class(b) && a.nblk == b.nblk && a.npart == b.npart && a.nblk_ax == b.nblk_ax && a.jgroups == b.jgroups &&
         a.nblk_u == b.nblk_u && a.npart_u == b.npart_u && a.nblk4 == b.nblk4 && a.nn_cap == b.nn_cap && a.ldp == b.ldp &&
         a.pstride == b.pstride && a.ld == b.ld && a.bytes.total() == b.bytes.total();
}

// "key":<integer> before the row's launches
static bool field(const std::string& head, const char* key, long long* v) {
  const std::string k = std::string("\"") + key + "\":";
  const size_t p = head.find(k);
  if (p == std::string::npos) return false;
  size_t q = p + k.size();
  if (head[q] == '"') ++q;   // knobs are recorded as strings
  char* end = nullptr;
  *v = strtoll(head.c_str() + q, &end, 10);
  return end != head.c_str() + q;
}
static void knob(const std::string& head, const char* name, shapes::Knob& kn) {
  long long v;
  if (field(head, name, &v)) kn = {true, (int64_t)v};
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s broyden_schedule.json\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::string text;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
  fclose(f);
  int rows = 0;
  for (size_t at = 0; at < text.size();) {   // one row per line
    size_t eol = text.find('\n', at);
    if (eol == std::string::npos) eol = text.size();
    const std::string line = text.substr(at, eol - at);
    at = eol + 1;
    const size_t it = line.find("\"iters\":");
    if (line.compare(0, 9, "{\"case\":\"") != 0 || it == std::string::npos) continue;
    const std::string head = line.substr(0, it);
    g_case = head.substr(9, head.find('"', 9) - 9);
    long long M, hint, thr, hist, keep, nodes, tiles;
    if (!(field(head, "M", &M) && field(head, "size_hint", &hint) && field(head, "thr", &thr) && field(head, "hist", &hist) &&
          field(head, "keep_trace", &keep) && field(head, "plan_nodes", &nodes) && field(head, "n_tiles", &tiles))) {
      fail("row without its inputs");
      continue;
    }
    Knobs kn;
    knob(head, "PSIGNN_VEC16_MIN", kn.vec16_min);
    knob(head, "PSIGNN_JGROUPS", kn.jgroups);
    knob(head, "PSIGNN_VEC_AX4", kn.vec_ax4);
    knob(head, "PSIGNN_UVU", kn.uvu);
    knob(head, "PSIGNN_U2D_KMAX", kn.u2d_kmax);
    knob(head, "PSIGNN_U2D_KEEP", kn.u2d_keep);
    const size_t form = head.find("\"PSIGNN_U2D_FORM\":\"");
    if (form != std::string::npos) kn.u2d_lds = {true, head[form + 19] == 'l' ? 1 : 0};
    BroydenShape sh = shapes::broyden_shape(M, hint, (int)thr, (int)hist, (int)keep, nodes, tiles, kn);
    run(sh, M, (int)hist, true);
    ++rows;
    if (sh.wants_big_lds()) {   // the same handle on a device that refuses the LDS attribute
      sh.cap_to_default_lds();
      g_case += " (64 KB of LDS)";
      run(sh, M, (int)hist, false);
    }
  }
  // the fold's limits in the LDS form: 38 / 36 is 31 / 31
  g_case = "lds 38/36";
  Knobs ask, cap;
  ask.u2d_lds = cap.u2d_lds = {true, 1};
  ask.u2d_kmax = {true, 38};
  ask.u2d_keep = {true, 36};
  cap.u2d_kmax = cap.u2d_keep = {true, 31};
  for (int64_t M : {(int64_t)1000000, (int64_t)3200000}) {
    const BroydenShape a = shapes::broyden_shape(M, 0, 48, 0, 1, 0, 0, ask), b = shapes::broyden_shape(M, 0, 48, 0, 1, 0, 0, cap);
    if (!same_shape(a, b) || a.u2d_kmax != 31 || a.u2d_keep != 31 || a.u2d_reg) fail("a request of 38 / 36 is not the shape of 31 / 31", a.u2d_kmax, a.u2d_keep);
    if (run(a, M, 0, false) != run(b, M, 0, false)) fail("a request of 38 / 36 does not run the schedule of 31 / 31");
  }
  if (rows == 0) {
    g_case = "table";
    fail("no row in the table");
  }
  printf("%s: %d cases, %d failures\n", g_bad ? "FAILED" : "ok", rows, g_bad);
  return g_bad ? 1 : 0;
}
