"""Two ranks on one GPU for tests/test_gpu_adi_res.py: the drop-in's Lyapunov solve in sweep form with the residual
rule, the sweeps sharded by shift inside the library (gloo callback).  Every rank writes its stopping step, rule and
residual history to ``<outdir>/rank<r>.npz``.
    python tests/adi_res_ranks.py <outdir>"""
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TOL = 1e-4


def worker(rank, world, port, out):
    import numpy as np
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        import sadptprj_riclyap_adi.proj_ric_utils as pru
        from optconpy_amd import backend
        from test_gpu_adi_res import MS, STEPS, lyap_inputs
        pr, F, W = lyap_inputs()
        res = pru.solve_proj_lyap_stein(amat=F, mmat=pr.M, jmat=pr.J, wmat=W,
                                        adi_dict=dict(ms=MS, adi_max_steps=STEPS, adi_newZ_reltol=0.0,
                                                      adi_res_reltol=TOL, sweep_width=16))
        sharded = getattr(backend.context(), "_xchg", None) is not None
        np.savez(os.path.join(out, "rank%d.npz" % rank), steps=res["adi_steps"], rule=res["adi_stopped_by"],
                 hist=res["adi_res_hist"], tol=TOL, sharded=int(sharded))
        backend.reset()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(worker, args=(2, port, sys.argv[1]), nprocs=2, join=True)
