"""Where should the multigrid's fused tail begin?  The ψ solve of the stream function - vorticity step (shape C of
scripts/bench_streamvorticity.py, BE, precond="mg") timed with different PG_MG_TAIL_ROWS: levels of at most that many rows run
in the one-workgroup tail kernel (k_mg_tail), larger ones with one launch per phase.  The library reads its configuration once
per process, so every threshold runs in a child process; windows of the thresholds alternate.

    python scripts/sweep_mg_tail.py [out.json] [n=1024] [thresholds: 0 300 1100]
    python scripts/sweep_mg_tail.py --worker n steps        (one process: prints one JSON line; also what the kernel trace runs)
"""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, ".")

WARMUP, STEPS, REPEATS = 5, 40, 3


def worker(n, steps):
    import numpy as np

    import penguin.jl_amd as pj

    pj.init(0)
    keys = ("left", "right", "bottom", "top")
    mesh = pj.Mesh((n, n), (1.0, 1.0), (0.0, 0.0))
    cap = pj.Capacity(pj.Sphere((0.5, 0.47), 0.15, complement=True), mesh)
    M = (n + 1) ** 2
    x, y = cap.C_ω[:, 0], cap.C_ω[:, 1]
    w0 = np.concatenate([20.0 * np.exp(-((x - 0.25) ** 2 + (y - 0.6) ** 2) / 0.01), np.zeros(M)])
    s = pj.StreamVorticity(cap, 1e-3, 0.32 / n, bc_stream=pj.Dirichlet(0.47),
                           bc_stream_border=pj.BorderConditions({k: pj.Dirichlet(lambda x, y, t=0.0: y) for k in keys}),
                           bc_vorticity_border=pj.BorderConditions({k: pj.Dirichlet(0.0) for k in keys}), ω0=w0)
    pj.run_StreamVorticity_b(s, WARMUP, "BE", save_every=0, precond="mg")
    pj.run_StreamVorticity_b(s, steps, "BE", save_every=0, precond="mg")
    r, info = s.last_run, s.psi_solver.mg_info()
    assert r.unconverged == 0
    print(json.dumps(dict(psi_ms_per_step=r.psi_ms / r.steps, psi_iters_per_step=r.psi_iters / r.steps, tail_level=info["tail_level"],
                          rows=info["rows"], tail_rows_env=os.environ.get("PG_MG_TAIL_ROWS", "default"))), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == "--worker":
    worker(int(sys.argv[2]), int(sys.argv[3]))
    sys.exit(0)

out = sys.argv[1] if len(sys.argv) > 1 else "profiles/mg_tail_sweep.json"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
thresholds = [int(a) for a in sys.argv[3:]] or [0, 300, 1100]
from penguin.jl_amd.build import source_hash

res = dict(what="ψ solve of the stream function - vorticity step with precond=mg against PG_MG_TAIL_ROWS", n=n, warmup_steps=WARMUP,
           steps_per_window=STEPS, windows=REPEATS, source_hash=source_hash(), thresholds=[])
runs = {t: [] for t in thresholds}
for _ in range(REPEATS):
    for t in thresholds:
        p = subprocess.run([sys.executable, __file__, "--worker", str(n), str(STEPS)], capture_output=True, text=True, timeout=280,
                           env={**os.environ, "PG_MG_TAIL_ROWS": str(t)})
        if p.returncode != 0:
            sys.exit(f"worker failed (threshold {t}): {p.stderr[-1500:]}")
        runs[t].append(json.loads(p.stdout.strip().splitlines()[-1]))
for t in thresholds:
    ms = [r["psi_ms_per_step"] for r in runs[t]]
    res["thresholds"].append(dict(tail_rows=t, tail_level=runs[t][0]["tail_level"], rows=runs[t][0]["rows"],
                                  rows_of_first_tail_level=runs[t][0]["rows"][runs[t][0]["tail_level"]],
                                  psi_iters_per_step=runs[t][0]["psi_iters_per_step"], psi_ms_per_step_windows=ms,
                                  psi_ms_per_step_median=statistics.median(ms)))
    print(json.dumps(res["thresholds"][-1]), flush=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
