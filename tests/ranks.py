"""How every multi-rank test starts its ranks and puts their maps together (a plain module, no fixtures).

launch() guarantees: each rank under its own time limit, the first failure ends the run, and no rank process or child of one is alive
when it returns.  cell_owner() and merge() are the "who owns which cell" array and the merged map of the raster tests."""
import os
import signal
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent

# One port per call site.  test_gpu_multirank.py's parametrised cases carry their ports in their test ids and stay in its parametrize
# lists; a second run of a case takes port + 1 and the retry port + 400.  tests/test_ranks_helper.py reads those lists and holds this
# table clear of them and of their offsets.
PORTS = {
    "rccl_refused": 29631, "no_finalize": 29632,        # test_gpu_multirank.py's two negative tests: no second run, no retry
    "partition_gloo": (29731, 29732, 29733),
    "output_maps": (29751, 29753),
    "snow": 29761, "crop": 29771, "root": 29773, "chain": 29775, "meteo": 29777, "sink": 29791, "rad": 29793, "rad_places": 29795,
}


def _killpg(p, sig):
    """Signals the rank's process group; False once the group has no member left (a zombie is one until it is reaped).  The group of a
    leader that is already reaped is signalled too - only so are children that outlived it reached - which counts on ProcessLookupError
    for an empty group and on its number not having been given to another group in between."""
    p.poll()
    try:
        os.killpg(p.pid, sig)
        return True
    except ProcessLookupError:
        return False


def _end(procs):
    """SIGTERM to every rank's process group, SIGKILL to those still there after 10 s: nothing of them stays alive"""
    for sig in (signal.SIGTERM, signal.SIGKILL):
        left = [p for p in procs if _killpg(p, sig)]
        end = time.monotonic() + 10.0
        while left and time.monotonic() < end:
            time.sleep(0.02)
            left = [p for p in left if _killpg(p, 0)]


def launch(worker, world, port, args, tmp_path, *, env=None, limit_s=240, wait_all=False, outfile=True):
    """`world` processes `timeout -k 10 <limit_s> python <worker> <rank> <world> <port> *args [<outfile>]`, each in a process group of its
    own, its output in a file under tmp_path.  Returns (returncodes, logs, outs).  The first rank that ends non-zero ends the run
    (wait_all=True: every rank runs to its own end, for the tests that expect a message from each).  No retry."""
    worker = ROOT / worker
    log_paths = [tmp_path / f"{worker.stem}_r{r}_{port}.log" for r in range(world)]
    outs = [lp.with_suffix(".npz") for lp in log_paths] if outfile else []
    # (ranks taking turns on one GPU: the exchange's 10 s bound is for ranks with a GPU each)
    full_env = {**os.environ, "SF3D_DIST_TIMEOUT_S": os.environ.get("SF3D_DIST_TIMEOUT_S", "60"), **(env or {})}
    procs = []
    try:
        for r in range(world):
            with open(log_paths[r], "w") as log:
                procs.append(subprocess.Popen(["timeout", "-k", "10", str(limit_s), sys.executable, str(worker), str(r), str(world), str(port),
                                               *map(str, args), *([str(outs[r])] if outfile else [])],
                                              stdout=log, stderr=subprocess.STDOUT, env=full_env, start_new_session=True))
        while True:
            codes = [p.poll() for p in procs]
            if None not in codes or (any(codes) and not wait_all):
                break
            time.sleep(0.02)
    finally:
        _end(procs)
    # 124 / 137: what `timeout -k` returns for a rank it had to end (137 is also any other SIGKILL of the rank, the OOM killer's for one)
    logs = [lp.read_text(errors="replace") + (f"\nrank {r}: time limit ({limit_s} s)" if p.returncode in (124, 137) else "")
            for r, (p, lp) in enumerate(zip(procs, log_paths))]
    return [p.returncode for p in procs], logs, outs


def run(worker, world, port, args, tmp_path, **kw):
    """launch(); fails the test with the logs unless every rank returned 0; the ranks' result files, loaded"""
    returncodes, logs, outs = launch(worker, world, port, args, tmp_path, **kw)
    if any(returncodes):
        pytest.fail("\n".join(f"--- rank {r}: exit {rc}\n{log}" for r, (rc, log) in enumerate(zip(returncodes, logs))))
    return [np.load(o) for o in outs]


def cell_owner(ranks, cell_node, n_nodes):
    """The rank that owns every cell: the owner of `cell_node`, the cell's surface node (-1: no node).  A node is owned by the rank
    whose own `owner` array claims it (a strip-local build knows the owner of the nodes it staged only); 255 where nobody does."""
    owner = np.full(n_nodes, 255, np.int64)
    for r, res in enumerate(ranks):
        owner[res["owner"] == r] = r
    cell_node = np.asarray(cell_node)
    cells = np.where(cell_node >= 0, owner[np.maximum(cell_node, 0)], 255)
    assert set(np.unique(cells[cell_node >= 0])) == set(range(len(ranks))), "every cell with a node has an owner and every rank owns cells"
    return cells


def merge(per_rank_arrays, cell_owner, fill, others=None, what="map"):
    """Every cell from the rank that owns it, over the trailing raster axes; `fill` where no rank owns the cell.  With `others`:
    every rank must hold exactly `others` on the cells that are not its own."""
    first = np.asarray(per_rank_arrays[0])
    merged = np.full(first.shape, fill, first.dtype)
    for r, a in enumerate(per_rank_arrays):
        mine = cell_owner == r
        if others is not None:
            assert np.all(a[..., ~mine] == others), f"{what}: rank {r} holds something else than {others} on another rank's cells"
        merged[..., mine] = a[..., mine]
    return merged
