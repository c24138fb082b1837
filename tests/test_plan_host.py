"""The graph analysis of the device build (criteria3d_amd/csrc/sf3d_host_plan.inc) without a device.  tests/plan_host.cpp includes that file
after sf3d_model.h - no HIP header - builds small models with links in setNodeLink's insertion order and holds every stage's claims against
the link data, node by node (see its head); here it is compiled and run, plainly and as a stand-alone program under the address and
undefined-behaviour sanitizers.

The shapes are the smallest on which each stage can still go wrong: the box 64 x 6 x 2 (the smallest grid the recogniser takes; every row
is an edge row or next to one, so slot alignment moves nodes in every chunk), the box 128 x 8 x 3 in one rank and cut for two (1 024 surface
nodes cut at 512, between rows 3 and 4: own rows, chunk lists with the owing chunks first, the directly addressed edge rows), the box
192 x 6 x 2 (the narrowest with a chunk away from both row ends: only there do all 64 codes of a chunk agree), a masked
outline of 70 x 7 cells with a hole and columns 2 and 3 layers deep (486 surface nodes, a short last chunk, a grid padded to 128 columns: the
masked recogniser, idxMap, the patch lists for W = 6 and 10, also cut mid-row for two ranks) and the first box with one lateral link
retargeted two columns away, which is neither.

The patch heights the program expects (256 compute units, no switch set) come from running the cost formula of plan_pair_patches by hand -
no fit is involved.  cost(W) = (1 + 0.6 / (W - 2)) * quant * (1 + 3.26 / (busyShare * wavesPerCU)) / sqrt(busyShare), with
perCU = 24 / (W + 1) blocks (3, 2, 1 at W = 6, 10, 14), resident = 256 perCU; W = 8 is only looked at when SF3D_PAIR_W asks for it:
  - 64 x 6: W = 6 alone fits 6 rows; 2 blocks on 2 of 256 units, 7 waves each: 1.15 * (1 + 3.26 / (7 / 128)) * sqrt(128) = 788
  - 128 x 8 (W = 10 needs 10 rows): 4 blocks, 1.15 * (1 + 3.26 / (7 / 64)) * 8 = 283; its strip of 4 rows has 2 blocks as the first box
  - the masked grid, 7 rows: 4 patches at W = 6, as the 128 x 8 box: 283
    all far above the threshold of 1.9 below the Infinity Cache: single sweeps (0); asked for (SF3D_PAIR_SWEEP=1), W = 6
  - 512 x 512 (C4): W = 6 1 024 blocks in two rounds of 768: 1.15 * 1.5 * (1 + 3.26 / 21) = 1.99; W = 10 512 blocks = one round:
    1.075 * (1 + 3.26 / 22) = 1.23; W = 14 344 blocks in two rounds of 256: 1.05 * 1.488 * (1 + 3.26 / 15) = 1.90: W = 10
  - one of eight strips of C4 (64 rows + 2 halo rows): W = 6 128 blocks on half the units: 1.15 * (1 + 3.26 / 3.5) * sqrt(2) = 3.14,
    W = 10 4.70, W = 14 5.24: single sweeps; asked for, W = 6"""
import re
import subprocess
from pathlib import Path

import pytest

from tests.raster_helpers import build_host_program

ROOT = Path(__file__).resolve().parent.parent
GROUPS = ["box 64 x 6 x 2", "refusal", "neither", "box 128 x 8 x 3", "box 192 x 6 x 2", "masked 70 x 7", "cost model", "step plan"]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_stage_holds_its_claims_against_the_link_data(tmp_path, sanitize):
    """the program has its own main and is not loaded into python; a failed claim or a sanitizer report ends it with a non-zero status"""
    run = subprocess.run([str(build_host_program("plan", tmp_path, sanitize))], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.splitlines() == [f"ok {g}" for g in GROUPS]


def test_plan_file_is_free_of_hip_and_of_the_environment():
    """what a stage reads from the environment or from the device arrives as an argument"""
    text = (ROOT / "criteria3d_amd" / "csrc" / "sf3d_host_plan.inc").read_text()
    assert re.findall(r"\bhip[A-Z_]\w*|\bgetenv\b|\bDeviceSolver\b|\bImpl\b|__global__|__device__", text) == []
