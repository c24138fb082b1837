"""tests/ranks.py on stand-in workers (plain python written into tmp_path: no torch, no GPU, no product library) and a hand-made raster."""
import os
import time

import numpy as np
import pytest

from tests import ranks

WRITER = """import sys
import numpy as np
rank, world, port, word, out = sys.argv[1:]
print(f"rank {rank} of {world} on {port} says {word}")
np.savez(out, rank=int(rank))
"""

# rank 0 records its pid and a child's and sleeps; rank 1 exits 3 as soon as both are on record
SLEEPER = """import os, subprocess, sys, time
rank, pids = int(sys.argv[1]), sys.argv[4]
if rank != 0:
    while not (os.path.exists(pids + ".rank") and os.path.exists(pids + ".child")):
        time.sleep(0.01)
    print("rank 1 gives up")
    sys.exit(3)
child = subprocess.Popen([sys.executable, "-c", "import os, sys, time; open(sys.argv[1], 'w').write(str(os.getpid())); time.sleep(60)", pids + ".child"])
open(pids + ".rank", "w").write(str(os.getpid()))
time.sleep(60)
"""

STAGGERED = """import sys, time
rank = int(sys.argv[1])
time.sleep(0.5 * rank)
print(f"rank {rank} refuses")
sys.exit(5 + rank)
"""

CHATTY = """import sys
for _ in range(1024):
    print("x" * 1023)
print("done")
"""


def _worker(tmp_path, text):
    path = tmp_path / "stand_in_worker.py"
    path.write_text(text)
    return path


def _gone(pid_file, within_s=5.0):
    pid, end = int(pid_file.read_text()), time.monotonic() + within_s
    while time.monotonic() < end:
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            return True
        time.sleep(0.02)
    return False


def test_all_ranks_succeed(tmp_path):
    res = ranks.run(_worker(tmp_path, WRITER), 2, 29901, ["hello"], tmp_path)
    assert [int(r["rank"]) for r in res] == [0, 1]
    for r in range(2):
        assert (tmp_path / f"stand_in_worker_r{r}_29901.log").read_text() == f"rank {r} of 2 on 29901 says hello\n"


def test_first_failure_ends_the_run(tmp_path):
    worker = _worker(tmp_path, SLEEPER)
    t = time.monotonic()
    returncodes, logs, outs = ranks.launch(worker, 2, 29902, [tmp_path / "pids"], tmp_path, outfile=False)
    assert time.monotonic() - t < 5.0
    assert returncodes[1] == 3 and returncodes[0] != 0 and "rank 1 gives up" in logs[1] and outs == []
    assert _gone(tmp_path / "pids.rank") and _gone(tmp_path / "pids.child")
    with pytest.raises(pytest.fail.Exception, match="rank 1: exit 3"):
        ranks.run(worker, 2, 29903, [tmp_path / "pids2"], tmp_path, outfile=False)


def test_time_limit(tmp_path):
    returncodes, logs, _ = ranks.launch(_worker(tmp_path, SLEEPER), 1, 29904, [tmp_path / "pids"], tmp_path, limit_s=1, outfile=False)
    assert returncodes[0] in (124, 137) and logs[0].endswith("rank 0: time limit (1 s)")
    assert _gone(tmp_path / "pids.rank") and _gone(tmp_path / "pids.child")


def test_wait_all_lets_every_rank_end_by_itself(tmp_path):
    returncodes, logs, _ = ranks.launch(_worker(tmp_path, STAGGERED), 2, 29905, [], tmp_path, wait_all=True, outfile=False)
    assert returncodes == [5, 6] and logs == ["rank 0 refuses\n", "rank 1 refuses\n"]


def test_a_chatty_rank_does_not_block(tmp_path):
    returncodes, logs, _ = ranks.launch(_worker(tmp_path, CHATTY), 1, 29906, [], tmp_path, limit_s=20, outfile=False)
    assert returncodes == [0] and len(logs[0]) > 2**20 and logs[0].endswith("done\n")


def test_ports_are_pairwise_different_and_clear_of_the_multirank_offsets():
    # what test_gpu_multirank.py's parametrised cases reach: their port, + 1 for a second run, + 400 for the retry, + 20 / + 40 in the two tests
    # with a third run (held against the other files only: its own two negative tests lie between its ports, and its tests run in turn)
    from tests import test_gpu_multirank as tm
    third = {"test_sharded_run_matches_oracle": (20,), "test_paired_sweep_on_strips_is_bitwise_the_single_sweeps": (40,)}      # (must follow that file)
    ports, reached = set(), set()
    for name, fn in vars(tm).items():
        for mark in getattr(fn, "pytestmark", []) if name.startswith("test_") else []:
            if mark.name == "parametrize" and "port" in mark.args[0].split(","):
                mine = {row[mark.args[0].split(",").index("port")] for row in mark.args[1]}
                ports |= mine
                reached |= {p + off for p in mine for off in (0, 1, 400) + third.get(name, ())}
    assert len(ports) > 30 and {29611, 29618, 29657, 29697} <= ports and {29638, 29697, 30097} <= reached
    own = {ranks.PORTS["rccl_refused"], ranks.PORTS["no_finalize"]}
    flat = [p for v in ranks.PORTS.values() for p in (v if isinstance(v, tuple) else (v,))]
    assert len(set(flat)) == len(flat)
    assert not own & {p + off for p in ports for off in (0, 1, 400)}
    assert not (set(flat) - own) & reached


class TestOwnerAndMerge:
    # 3 x 4 cells, nodes numbered row by row without the cell (1, 2); a second layer of 11 nodes below.  Rank 0 owns two rows, rank 1 the last
    cell_node = np.array([[0, 1, 2, 3], [4, 5, -1, 6], [7, 8, 9, 10]])
    node_owner = np.array([0] * 7 + [1] * 4 + [0] * 7 + [1] * 4)
    by_hand = np.array([[0, 0, 0, 0], [0, 0, 255, 0], [1, 1, 1, 1]])
    seen = [dict(owner=node_owner), dict(owner=np.where(np.arange(22) < 4, -1, node_owner))]      # (a strip-local build: -1 for nodes it never staged)

    def test_owner_as_written_by_hand(self):
        assert np.array_equal(ranks.cell_owner(self.seen, self.cell_node, 22), self.by_hand)
        assert np.array_equal(ranks.cell_owner(self.seen, np.arange(22), 22), self.node_owner)      # the nodes' owner: every node its own cell

    def test_merge_as_written_by_hand(self):
        a = [np.full((2, 3, 4), -9.0), np.full((2, 3, 4), -9.0)]
        a[0][:, :2] = [[1, 2, 3, 4], [5, 6, -9, 7]]
        a[1][:, 2] = [8, 9, 10, 11]
        a[1][1, 2] *= 2
        want = np.array([[[1, 2, 3, 4], [5, 6, -9, 7], [8, 9, 10, 11]], [[1, 2, 3, 4], [5, 6, -9, 7], [16, 18, 20, 22]]], float)
        got = ranks.merge(a, self.by_hand, -9.0, others=-9.0)
        assert got.dtype == a[0].dtype and np.array_equal(got, want)
        assert np.array_equal(ranks.merge([x[0] for x in a], self.by_hand, 0.0)[1], [5, 6, 0, 7])      # the fill where nobody owns the cell

    def test_one_foreign_value_is_found(self):
        a = [np.full((3, 4), -9.0), np.full((3, 4), -9.0)]
        ranks.merge(a, self.by_hand, -9.0, others=-9.0)
        a[1][0, 3] = 0.5
        with pytest.raises(AssertionError, match="et0: rank 1"):
            ranks.merge(a, self.by_hand, -9.0, others=-9.0, what="et0")
        a[1][0, 3], a[0][1, 2] = -9.0, 0.5                              # the cell without a node is nobody's
        with pytest.raises(AssertionError, match="rank 0"):
            ranks.merge(a, self.by_hand, -9.0, others=-9.0)

    def test_a_rank_that_owns_nothing_is_refused(self):
        with pytest.raises(AssertionError):
            ranks.cell_owner([dict(owner=np.zeros(22, np.int64))] * 2, self.cell_node, 22)
