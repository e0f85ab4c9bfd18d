"""The workspace sizes a commit's *_workspace_floats queries return, as a table for tests/host/workspace_check.cpp.

Test infrastructure (build container only).  csrc/workspace.h computes every workspace size and layout with one builder; a
refactor of it must leave every number a query returns unchanged.  This script records those numbers from a BUILT checkout of the
commit to compare against (the parent of a change to workspace.h): it compiles a throw-away program against that tree's common.h
and shared libraries, which calls every query on a stub plan (only N and mixed are set; the queries read nothing else), at each
latent width the tree builds (10: every query; 8 and 16: the forward libraries, psignn_f_workspace_floats alone).

Output: tests/golden/workspace_sizes.json, a list with one flat record per line
    {"D": 10, "query": "f_param_vjp", "mixed": 0, "nl": 1, "N": 63, "floats": 62754}
(workspace_check.cpp reads it line by line).  No GPU is needed: the queries are host arithmetic.

    python oracle/make_golden_workspace_sizes.py --tree /path/to/built/checkout
"""
import argparse
import json
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 63, 64, 65, 257, 5329, 99919, 1000519]
NLS = [1, 2, 3, 64]

PROGRAM = r"""
#include "common.h"
#include <stdio.h>
int main() {
  const long long Ns[] = {%(ns)s};
  const int nls[] = {%(nls)s};
  for (long long N : Ns)
    for (int mixed = 0; mixed < 2; ++mixed) {
      psignn_plan p;
      p.N = N;
      p.mixed = mixed;
#define REC(q, nl, v) printf("{\"D\": %%d, \"query\": \"%%s\", \"mixed\": %%d, \"nl\": %%d, \"N\": %%lld, \"floats\": %%lld}\n", \
                             (int)PSIGNN_D, q, mixed, nl, N, (long long)(v))
      REC("f", 1, psignn_f_workspace_floats(&p));
#if PSIGNN_D == 10
      REC("f_param_vjp", 1, psignn_f_param_vjp_workspace_floats(&p));
      REC("f_vjp_backward", 1, psignn_f_vjp_backward_workspace_floats(&p));
      REC("f_vjp_backward_p", 1, psignn_f_vjp_backward_p_workspace_floats(&p));
      REC("dsgps_step_backward", 1, psignn_dsgps_step_backward_workspace_floats(&p));
      REC("dss_step_backward", 1, psignn_dss_step_backward_workspace_floats(&p));
      REC("mlp2_backward", 1, psignn_mlp2_backward_workspace_floats(N));
      for (int nl : nls) {
        REC("f_layers", nl, psignn_f_layers_workspace_floats(&p, nl));
        REC("gmres_adjoint", nl, psignn_gmres_adjoint_workspace_floats(&p, nl));
      }
#endif
    }
  return 0;
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="a built checkout of the commit whose numbers are recorded")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "workspace_sizes.json"))
    a = ap.parse_args()
    pkg = os.path.join(os.path.abspath(a.tree), "psi-gnn_amd")
    src = PROGRAM % {"ns": ", ".join(map(str, NS)), "nls": ", ".join(map(str, NLS))}
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        cpp = os.path.join(tmp, "sizes.hip")
        with open(cpp, "w") as f:
            f.write(src)
        for d, lib in ((10, "psignn_hip"), (8, "psignn_hip_d8"), (16, "psignn_hip_d16")):
            exe = os.path.join(tmp, f"sizes_d{d}")
            subprocess.run([a.hipcc, "--offload-arch=gfx950", "-std=c++17", f"-DPSIGNN_D={d}", "-I", os.path.join(pkg, "csrc"), cpp,
                            "-o", exe, "-L", pkg, f"-l{lib}", f"-Wl,-rpath,{pkg}"], check=True)
            lines += subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    for ln in lines:
        json.loads(ln)
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(lines) + "\n]\n")
    print(f"{len(lines)} records -> {a.out}")


if __name__ == "__main__":
    main()
