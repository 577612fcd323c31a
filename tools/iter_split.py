"""Wall time of one hot lockstep GMRES iteration on one stream against the same batch as two half-batches on two
streams (ricadi_time_kernel_dev classes iter / iter_split), for ng = 16, 8, 4, 2 groups of width 16.
python tools/iter_split.py [N ...]     (default: 58 = cfg2, 236 = cfg5; N = 236 with convection, as bench.py)
One JSON line per (N, ng) on stdout.  With --trace-only N ng: form iter_split alone, for rocprofv3 --kernel-trace."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from optconpy_amd import _lib, problems as pb  # noqa: E402


def context(N):
    pr = pb.ricc_problem(N, 0.05, with_convection=(N == 236))
    ctx = _lib.Context(0)
    ctx.set_operator((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J)
    return ctx


def main():
    torch.cuda.set_device(0)
    ms = list(pb.logshifts(1.0, 3e3, 16))
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-only":
        N, ng = int(sys.argv[2]), int(sys.argv[3])
        ctx = context(N)
        for name in ("iter", "iter_split"):
            ctx.time_kernel_dev(name, ms[:ng], [1.0] * ng, 16, nvec=7, reps=20)
        ctx.close()
        return
    for N in [int(a) for a in sys.argv[1:]] or [58, 236]:
        ctx = context(N)
        reps = 50 if N < 100 else 10
        for ng in (16, 8, 4, 2):
            al, be = ms[:ng], [1.0] * ng
            t = {"iter": [], "iter_split": []}
            for name in t:
                ctx.time_kernel_dev(name, al, be, 16, nvec=7, reps=3)     # warm-up
            for trial in range(5):                                        # alternated
                for name in (("iter", "iter_split") if trial % 2 == 0 else ("iter_split", "iter")):
                    t[name].append(1e3 * ctx.time_kernel_dev(name, al, be, 16, nvec=7, reps=reps))
            one, two = float(np.median(t["iter"])), float(np.median(t["iter_split"]))
            print(json.dumps(dict(N=N, ng=ng, us_one_stream=round(one, 1), us_two_streams=round(two, 1),
                                  gain=round(1.0 - two / one, 4), trials_one=[round(x, 1) for x in t["iter"]],
                                  trials_two=[round(x, 1) for x in t["iter_split"]])), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
