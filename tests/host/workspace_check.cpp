// Stand-alone check of csrc/workspace.h (host only; build with -fsanitize=address,undefined and run on its own):
//   workspace_check tests/golden/workspace_sizes.json        compiled once per latent width (-DPSIGNN_D=8|10|16)
// For every layout, at N in {1, 63, 64, 65, 257, 5329, 99919, 1000519}, n_layers in {1, 2, 3, 64} and both families:
//   * every segment lies inside [0, total) with the size its kernels need (stated here, independently of the header),
//   * segments that are not declared aliases do not overlap,
//   * every segment offset is even (rows move as float2),
//   * total equals the recorded value of the query (workspace_sizes.json: one flat record per line), and a view carved inside
//     another layout fills exactly the region it is given.
// Prints the totals it computed as records of the same form (the pytest test compares them with the table) and exits non-zero
// on the first layout that fails.  Nothing is allocated: the segments are offsets from a base that is never dereferenced.
#include "workspace.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

static float* const BASE = reinterpret_cast<float*>(uintptr_t(1) << 40);
static const int64_t D = ws::W;
static int g_bad = 0;

struct Seg {
  const char* name;
  const float* p;
  int64_t size;
  bool alias;   // declared to share storage with other segments of the layout
};
struct Rec {
  std::string query;
  int mixed, nl;
  int64_t N, floats;
};
static std::vector<Rec> g_table, g_seen;

static void fail(const char* layout, int64_t N, int nl, int mixed, const char* what, const char* seg = "") {
  printf("FAIL D=%d %s N=%lld nl=%d mixed=%d: %s %s\n", (int)D, layout, (long long)N, nl, mixed, what, seg);
  ++g_bad;
}
// base: where the layout was carved (inside BASE's region); total: the region's size
static void check(const char* layout, int64_t N, int nl, int mixed, const float* base, int64_t total, const std::vector<Seg>& segs) {
  for (size_t i = 0; i < segs.size(); ++i) {
    const Seg& s = segs[i];
    const int64_t o = s.p - base;
    if (s.size < 0 || o < 0 || o + s.size > total || (s.size > 0 && o >= total)) fail(layout, N, nl, mixed, "outside [0, total):", s.name);
    if ((s.p - BASE) & 1) fail(layout, N, nl, mixed, "odd offset:", s.name);
    for (size_t j = 0; j < i; ++j) {
      const Seg& t = segs[j];
      if (s.alias || t.alias || s.size == 0 || t.size == 0) continue;
      if (s.p < t.p + t.size && t.p < s.p + s.size) fail(layout, N, nl, mixed, "overlap:", s.name);
    }
  }
}
// a root layout: total against the recorded query
static void expect(const char* query, int64_t N, int nl, int mixed, int64_t total) {
  g_seen.push_back({query, mixed, nl, N, total});
  printf("{\"D\": %d, \"query\": \"%s\", \"mixed\": %d, \"nl\": %d, \"N\": %lld, \"floats\": %lld}\n", (int)D, query, mixed, nl,
         (long long)N, (long long)total);
  if (total & 1) fail(query, N, nl, mixed, "odd total (a workspace appended to it would start on an odd offset)");
  for (const Rec& r : g_table)
    if (r.query == query && r.N == N && r.nl == nl && r.mixed == mixed) {
      if (r.floats != total) fail(query, N, nl, mixed, "total differs from the recorded value");
      return;
    }
  fail(query, N, nl, mixed, "no recorded value");
}
// partial tiles of the reduction kernels (fgnn_pgrad.hip k_pgrad_outer): a wave owns max(64, a multiple of 4) records, a block 4
// waves; one set of nt tiles per block for nt <= 16, one per wave beyond
static int64_t parts(int64_t n, int nt) {
  int64_t npw = (((n + 4095) / 4096) + 3) / 4 * 4;
  if (npw < 64) npw = 64;
  const int64_t nblk = (n + npw * 4 - 1) / (npw * 4);
  return nblk * (nt <= 16 ? 1 : 4) * nt * 256;
}
static std::vector<Seg> jr_scratch_segs(int64_t N, int mixed, float* base) {
  const ws::JrScratch s = ws::jr_scratch(N, mixed, base);
  const int64_t ND = N * D, w = mixed ? 6 : 4;
  return {{"P", s.P, w * ND, false}, {"cb", s.cb, 4 * ND, false}, {"B", s.B, w * ND, false}, {"dir", s.dir, ND, false}};
}

static void check_forward(int64_t N, int mixed) {   // the layouts every width has
  const int64_t ND = N * D, F = ws::f_total(N);
  expect("f", N, 1, mixed, F);
  const ws::FFwd g = ws::f_fwd(N, false, BASE, F);
  check("f_fwd gather", N, 1, mixed, BASE, g.total, {{"Pj", g.Pj, 6 * ND, false}, {"pp0", g.pp[0], ND, false}, {"pp1", g.pp[1], ND, false},
                                                     {"spare", g.spare, F - (g.spare - BASE), false}});
  if (g.total != F) fail("f_fwd gather", N, 1, mixed, "total");
  const ws::Adapter a = ws::f_adapter(N, false, BASE);
  check("f_adapter", N, 1, mixed, BASE, a.total, {{"h", a.h, ND, false}, {"x", a.x, ND, false}, {"out", a.out, ND, false},
                                                  {"prb", a.prb, 3 * N, false}, {"nrm", a.nrm, 2 * N, false}, {"rest", a.rest, a.rest_floats, false}});
  if (a.total != F || a.rest_floats < 0) fail("f_adapter", N, 1, mixed, "total");
  const ws::FFwd t = ws::f_fwd(N, true, a.rest, a.rest_floats);   // the tile forward behind the adapter
  check("f_fwd tiles", N, 1, mixed, a.rest, a.rest_floats, {{"pp0", t.pp[0], ND, false}, {"pp1", t.pp[1], ND, false}});
  if (t.total != a.rest_floats) fail("f_fwd tiles", N, 1, mixed, "does not fit the adapter's rest");
}

static void check_derivatives(int64_t N, int mixed, int nl) {   // width 10
  const int64_t ND = N * D, F = ws::f_total(N), rec = N * (mixed ? 480 : 320);
  if (nl == 1) {
    const ws::FVjp v = ws::f_vjp(N, mixed, BASE, F);
    check("f_vjp", N, nl, mixed, BASE, v.total, {{"Pj", v.Pj, (mixed ? 3 : 2) * ND, false}, {"B", v.B, (mixed ? 6 : 4) * ND, false}});
    if (v.total != F) fail("f_vjp", N, nl, mixed, "total");
    for (int adjoint = 0; adjoint < 2; ++adjoint) {
      const ws::Adapter a = adjoint ? ws::f_adjoint(N, BASE) : ws::f_adapter(N, true, BASE);
      check(adjoint ? "f_adjoint" : "f_adapter B", N, nl, mixed, BASE, a.total,
            {{"B", a.B, 4 * ND, false}, {"h", a.h, ND, false}, {"x", a.x, ND, false}, {"out", a.out, adjoint ? 0 : ND, false},
             {"prb", a.prb, adjoint ? 0 : 3 * N, false}, {"nrm", a.nrm, adjoint ? 0 : 2 * N, false}});
      if (a.total != F) fail("f_adapter B", N, nl, mixed, "total");
    }
    // parameter VJP: the gather form, the plan-order tile form, the caller-order adapter with either behind it
    const int64_t PV = ws::pv_total(N);
    expect("f_param_vjp", N, nl, mixed, PV);
    for (int rows : {9, 4}) {
      const ws::RecWork w = ws::pv_work(N, mixed, rows, BASE, PV);
      check("pv_work", N, nl, mixed, BASE, w.total, {{"scratch", w.scratch, rows * ND, false}, {"rec", w.rec, rec, false},
                                                     {"part", w.part, parts(N, mixed ? 24 : 16), false}, {"spare", w.spare, PV - (w.spare - BASE), false}});
      if (w.total != PV) fail("pv_work", N, nl, mixed, "total");
      const ws::FVjp v9 = ws::f_vjp(N, mixed, w.scratch, rows * ND);
      if (rows == 9 && v9.total != 9 * ND) fail("pv_work", N, nl, mixed, "the gather VJP's Pj | B do not fit the scratch");
      const ws::Adapter a = ws::pv_adapter(N, mixed, BASE);
      check("pv_adapter", N, nl, mixed, BASE, a.total, {{"h", a.h, ND, false}, {"x", a.x, ND, false}, {"out", a.out, ND, false},
                                                        {"prb", a.prb, (mixed ? 3 : 2) * N, false}, {"nrm", a.nrm, mixed ? 2 * N : 0, false},
                                                        {"rest", a.rest, a.rest_floats, false}});
      if (a.total != PV || ((a.rest - BASE) & 3)) fail("pv_adapter", N, nl, mixed, "total, or rest not on a multiple of four");
      const ws::RecWork n = ws::pv_work(N, mixed, rows, a.rest, a.rest_floats);
      check("pv_work behind the adapter", N, nl, mixed, a.rest, a.rest_floats,
            {{"scratch", n.scratch, rows * ND, false}, {"rec", n.rec, rec, false}, {"part", n.part, parts(N, mixed ? 24 : 16), false}});
      if (n.total != a.rest_floats) fail("pv_work behind the adapter", N, nl, mixed, "does not fit the adapter's rest");
    }
    // backward of the VJP: gather form with the scratch of gather_backward.hip inside, plan-order tile form
    const ws::JrWork j = ws::jr_work(N, mixed, false, BASE);
    expect("f_vjp_backward", N, nl, mixed, j.total);
    check("jr_work", N, nl, mixed, BASE, j.total,
          {{"scratch", j.scratch, 17 * ND, false}, {"rec1", j.rec1, rec, false}, {"rec2", j.rec2, rec, false},
           {"part2", j.part2, parts(2 * N, mixed ? 24 : 16), false}, {"spare", j.spare, j.total - (j.spare - BASE), false},
           {"part1", j.part1, mixed ? 0 : parts(N, 16), true}});
    if (j.part1 != j.rec2) fail("jr_work", N, nl, mixed, "part1 is declared to start where rec2 does");
    check("jr_scratch", N, nl, mixed, j.scratch, 17 * ND, jr_scratch_segs(N, mixed, j.scratch));
    const ws::JrWork t = ws::jr_work(N, false, true, BASE);
    expect("f_vjp_backward_p", N, nl, mixed, t.total);
    check("jr_work tiles", N, nl, mixed, BASE, t.total, {{"B", t.scratch, 6 * ND, false}, {"rec1", t.rec1, N * 320, false},
                                                          {"rec2", t.rec2, N * 320, false}, {"part", t.part2, parts(2 * N, 16), false}});
    // DS-GPS / DSS step backward, MLP backward
    const ws::RecWork g = ws::dsgps_bw_work(N, mixed, BASE);
    expect("dsgps_step_backward", N, nl, mixed, g.total);
    check("dsgps_bw_work", N, nl, mixed, BASE, g.total, {{"scratch", g.scratch, 17 * ND, false}, {"rec", g.rec, rec, false},
                                                         {"part", g.part, parts(N, mixed ? 27 : 19), false}, {"spare", g.spare, g.total - (g.spare - BASE), false}});
    check("jr_scratch (dsgps)", N, nl, mixed, g.scratch, 17 * ND, jr_scratch_segs(N, mixed, g.scratch));
    const ws::RecWork s = ws::dss_bw_work(N, BASE);
    expect("dss_step_backward", N, nl, mixed, s.total);
    check("dss_bw_work", N, nl, mixed, BASE, s.total, {{"scratch", s.scratch, 13 * ND, false}, {"rec", s.rec, N * 320, false}, {"part", s.part, parts(N, 16), false}});
    check("jr_scratch (dss)", N, nl, mixed, s.scratch, 13 * ND, jr_scratch_segs(N, 0, s.scratch));
    const ws::RecWork m = ws::mlp2_bw_work(N, BASE);
    expect("mlp2_backward", N, nl, mixed, m.total);
    check("mlp2_bw_work", N, nl, mixed, BASE, m.total, {{"rec", m.rec, N * 64, false}, {"part", m.part, parts(N, 2), false}});
    // DS-GPS / DSS forward: the documented sizes
    const ws::DsgpsWork dg = ws::dsgps_work(N, mixed, BASE);
    check("dsgps_work", N, nl, mixed, BASE, dg.total, {{"h0", dg.h0, ND, false}, {"a", dg.a, ND, false}, {"b", dg.b, ND, false},
                                                       {"prb", dg.prb, (mixed ? 3 : 2) * N, false}, {"nrm", dg.nrm, mixed ? 2 * N : 0, false}});
    if (dg.total != 4 * ND) fail("dsgps_work", N, nl, mixed, "total is documented as 4 * N * 10");
    const ws::DssWork ds = ws::dss_work(N, BASE);
    check("dss_work", N, nl, mixed, BASE, ds.total, {{"a", ds.a, ND, false}, {"b", ds.b, ND, false}, {"bprime", ds.bprime, 3 * N, false}});
    if (ds.total != 23 * N) fail("dss_work", N, nl, mixed, "total is documented as N * 23");
  }
  // layer workspace: its two readings of the rows
  const ws::LayerWork L = ws::layer_work(N, nl, mixed, BASE);
  expect("f_layers", N, nl, mixed, L.total);
  const int64_t view = nl > 1 ? 4096 : 0;
  if (nl > 1 && !mixed) {
    check("layer_work chains", N, nl, mixed, BASE, L.total, {{"S", L.S, (nl - 1) * ND, false}, {"tb0", L.tb[0], ND, false}, {"tb1", L.tb[1], ND, false},
                                                             {"init", L.init, ND, false}, {"view", L.view, view, false}});
    check("layer_work backward of the VJP", N, nl, mixed, BASE, L.total,
          {{"S", L.S, (nl - 1) * ND, false}, {"Wc", L.Wc, (nl - 1) * ND, false}, {"G", L.G, (nl - 1) * ND, false}, {"C", L.C, nl * ND, false},
           {"A", L.A, 2 * ND, false}, {"T", L.T, ND, false}, {"view", L.view, view, false}});
    if (L.state(1) != L.S || (nl > 2 && L.state(2) != L.S + ND)) fail("layer_work", N, nl, mixed, "state(k)");
  } else {
    check("layer_work view", N, nl, mixed, BASE, L.total, {{"view", L.view, view, false}});
  }
  // GMRES adjoint solve
  const ws::AdjWork w = ws::adj_work(N, nl, mixed, BASE);
  expect("gmres_adjoint", N, nl, mixed, w.total);
  const std::vector<Seg> segs = {{"fwork", w.fwork, F, false}, {"y", w.y, ND, false}, {"fy", w.fy, ND, false}, {"ybest", w.ybest, ND, false},
                                 {"grad_p", w.grad_p, ND, false}, {"hs_p", w.hs_p, ND, false}, {"prbp", w.prbp, 3 * N, false},
                                 {"nrmp", w.nrmp, 2 * N, false}, {"lwork", w.lwork, mixed ? 0 : L.total, false}};
  check("adj_work", N, nl, mixed, BASE, w.total, segs);
  for (const Seg& s : segs)
    if ((s.p - BASE) % 64) fail("adj_work", N, nl, mixed, "segment not on a 256-byte boundary:", s.name);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s workspace_sizes.json\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char line[512], query[64];
  while (fgets(line, sizeof line, f)) {
    int d, mixed, nl;
    long long N, floats;
    if (sscanf(line, " {\"D\": %d, \"query\": \"%63[^\"]\", \"mixed\": %d, \"nl\": %d, \"N\": %lld, \"floats\": %lld}", &d, query, &mixed, &nl, &N,
               &floats) == 6 && d == (int)D)
      g_table.push_back({query, mixed, nl, (int64_t)N, (int64_t)floats});
  }
  fclose(f);
  const int64_t Ns[] = {1, 63, 64, 65, 257, 5329, 99919, 1000519};
  const int nls[] = {1, 2, 3, 64};
  for (int64_t N : Ns)
    for (int mixed = 0; mixed < 2; ++mixed) {
      check_forward(N, mixed);
      if (D == 10)
        for (int nl : nls) check_derivatives(N, mixed, nl);
    }
  for (const Rec& r : g_table) {   // every recorded value of this width was compared
    bool seen = false;
    for (const Rec& s : g_seen) seen = seen || (s.query == r.query && s.N == r.N && s.nl == r.nl && s.mixed == r.mixed);
    if (!seen) fail(r.query.c_str(), r.N, r.nl, r.mixed, "recorded value was not checked");
  }
  if (g_table.empty()) fail("table", 0, 0, 0, "no record of this width in the table");
  printf("%s: D=%d, %zu totals, %d failures\n", g_bad ? "FAILED" : "ok", (int)D, g_seen.size(), g_bad);
  return g_bad ? 1 : 0;
}
