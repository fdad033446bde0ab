"""One rank of the two-process SyncBN test (tests/test_gpu_batchnorm.py).

Launched by the test as a child process per rank (never an exec of the test
process), both ranks on cuda:0, torch.distributed over gloo.  Each rank runs
one forward + backward of a sync=True batch-statistics BatchNorm on ITS OWN
rows ([1,5,7,8] and [1,3,4,8]: unequal counts) on the HIP arm and saves every
result with the names of the launches it recorded.

    python tests/bn_sync_worker.py <outdir>        (RANK / WORLD_SIZE / MASTER_* in env)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main(out):
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd.layers.ops import KernelTimer
    from test_batchnorm_cpu import run_layer, sync_inputs
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    _C.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ts, _ = sync_inputs()
    KernelTimer.reset()
    got = run_layer(ts[rank], dev, sync=True)
    names = [r[0] for r in KernelTimer.records]
    KernelTimer.reset(enabled=False)
    _C.raise_on_errors(dev)
    rec = {k: (v if v is None else v.cpu()) for k, v in got.items()}
    rec["launches"] = names
    torch.save(rec, os.path.join(out, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
