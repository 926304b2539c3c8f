"""Worker of test_layered_data_parallel_gradients_equal_full_batch: one rank of a data-parallel GaugeTrainer step on a
6x6 lattice, which takes the layered training path.  Each rank owns a contiguous shard of the chains; rank 0 saves the
gradients of the bucketed exchange and of one all-reduce of the whole buffer."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_gpu_gauge_train_layered import _setup_tx  # noqa: E402
from l2hmc_amd.dist import shard_bounds  # noqa: E402


def main():
    out, B = sys.argv[1], int(sys.argv[2])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)            # the test box has one GPU: both ranks share it, gloo carries the exchange
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    tr, tm, x, z, dx, dz = _setup_tx(6, 6, 2, 0.2, B, "mild")
    lo, hi = shard_bounds(B, world, rank)
    tr = GaugeTrainer(tr.dynamics, dist=dist)           # bucketed (the default)
    assert tr.bucketed
    shard = dict(z=z[lo:hi], draws_x=tuple(a[lo:hi] for a in dx), draws_z=tuple(a[lo:hi] for a in dz))
    loss, *_ = tr.calc_loss_and_grads(x[lo:hi], 2.5, **shard)
    assert tr._walk is not None
    buckets = tr.last_bucket_count
    g_bucketed = tr.grads.cpu().numpy().copy()
    tr.bucketed = False                                 # one all-reduce of the whole buffer after the pass
    tr.calc_loss_and_grads(x[lo:hi], 2.5, **shard)
    g_single = tr.grads.cpu().numpy().copy()
    tr.apply_gradients()
    if rank == 0:
        np.savez(out, grads=g_bucketed, grads_single=g_single, loss=float(loss), lr=tr.learning_rate(),
                 buckets=buckets)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
