"""What the scripts/multirank_*_worker.py share: one rank of a multi-rank run of the HIP product whose ranks may share one GPU, with
torch.distributed (gloo) as the control plane.  A worker calls start(), builds its model with build(), does its module's part and ends
with finish().
command line of every worker: <rank> <world> <port> <number> <outfile>"""
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np                                          # noqa: E402
import torch.distributed as dist                            # noqa: E402
from criteria3d_amd import capi, catchment as cm, maps      # noqa: E402


def start():
    """joins the process group; returns (rank, world, number, outfile)"""
    rank, world, port, number, outfile = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, world, number, outfile


def allgather(b):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, b)
    return out


def build(m, columns=True, **kw):
    """the product on this rank's strip of `m`, with the bindings of include/sf3d_maps.h and (columns) the column table of `m` set"""
    sf = capi.load_product()
    sf.check(sf.lib.sf3d_set_device(int(os.environ.get("SF3D_TEST_DEVICE", "0"))), "set_device")
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1, dist=(dist.get_rank(), dist.get_world_size(), allgather), **kw)
    maps.bind(sf)
    if columns:
        maps.set_columns(sf, *maps.columns(m))
    return sf


def surface_dem(m, flag):
    """the elevation of the surface node of every cell of a project model, `flag` where there is none"""
    idx = np.asarray(m.meta["index"])[0]
    return idx, np.where(idx >= 0, m.z[np.maximum(idx, 0)], flag).astype(np.float32)


def finish(sf, outfile, res):
    np.savez(outfile, **res)
    dist.barrier()
    sf.lib.sf3d_clean()
    dist.destroy_process_group()
