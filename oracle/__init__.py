"""CPU oracle of the PSI-GNN path (psignn_oracle) and the recipes of the golden vectors under tests/golden (make_golden*.py)."""

# fp32 CPU arithmetic that gives the same bits on every x86-64 host: MKL's processor-independent code path, ATen's
# non-vectorised kernels, one thread.  Read when MKL / ATen start, so it goes into a process's environment before torch
# is imported.  The fixtures that tests compare to fp32 rounding (broyden_ls.npz, dss_*.npz) are generated under it, and
# those tests recompute under it in a child process: their tolerances hold on any host, not only on the one that made them.
PINNED_CPU_ENV = {"MKL_CBWR": "COMPATIBLE", "ATEN_CPU_CAPABILITY": "default", "OMP_NUM_THREADS": "1", "MKL_NUM_THREADS": "1"}
