"""Parity tests proper: the HIP product (through the C ABI) against the CPU oracle on the same
inputs.  BASELINE.json's north_star asks for node H and the cumulative mass balance within 1e-6 relative;
the tests hold 1e-9 (tests/tolerances.py: the elementary functions are the reference C library's bit
for bit since round 5, only the reductions are tree- instead of index-ordered)."""
import numpy as np
import pytest

from criteria3d_amd import capi, catchment as cm
from tests.tolerances import WATER_RTOL, assert_water_nodes

pytestmark = pytest.mark.gpu

RTOL = WATER_RTOL    # north_star: node H and cumulative mass balance within 1e-6 relative; held: 1e-9 (tests/tolerances.py)


def rel(a, b, floor=1e-9):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))) if a.size else 0.0


def run_pair(product, oracle, model, forcing, hours, use_period=False):
    """Yield (hour, product snapshot, oracle snapshot, product dts, oracle dts)."""
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset_solver_state")
        cm.build(sf, model, threads=1)
    for h in range(hours):
        mm = cm.FORCINGS[forcing](h)
        out = []
        for sf in (product, oracle):
            steps, dts = cm.run_hour(sf, model, mm, use_period=use_period)
            out.append((cm.snapshot(sf, model), dts))
        yield h, out[0][0], out[1][0], out[0][1], out[1][1]


def assert_snapshot_close(g, o, tag):
    assert_water_nodes(g["H"], o["H"], f"{tag}: H")
    assert_water_nodes(g["Se"], o["Se"], f"{tag}: Se")
    for k in ("total_water", "storage"):
        assert abs(g[k] - o[k]) <= RTOL * abs(o[k]), f"{tag}: {k} {g[k]!r} vs {o[k]!r}"
    for k in ("runoff", "drainage", "lateral"):
        assert abs(g[k] - o[k]) <= RTOL * max(abs(o[k]), 1e-3), f"{tag}: {k} {g[k]!r} vs {o[k]!r}"


def test_column_c1_24h(product, oracle):
    """C1: 1-D column, 100 nodes, free drainage, constant rain, 24 h, via computeStep."""
    m = cm.column_model()
    for h, g, o, gd, od in run_pair(product, oracle, m, "R5", 24):
        assert len(gd) == len(od), f"hour {h}: accepted steps {len(gd)} vs {len(od)}"
        np.testing.assert_allclose(gd, od, rtol=1e-12)
        assert_snapshot_close(g, o, f"C1 h{h}")
    assert product.counters()["accepted"] == oracle.counters()["accepted"]


def test_column_c1_compute_period_mbr(product, oracle):
    """computePeriod updates the whole-period mass-balance ratio (water.cpp:143-156)."""
    m = cm.column_model()
    for h, g, o, _, _ in run_pair(product, oracle, m, "R5", 6, use_period=True):
        assert_snapshot_close(g, o, f"C1p h{h}")
        # MBR = (delta storage - cumulative sink) / max(1 litre, sink): a difference of nearly equal
        # numbers, so it is compared absolutely (it is judged against thresholds of 1e-3..1e-2)
        assert abs(g["mbr"] - o["mbr"]) <= 1e-6, (g["mbr"], o["mbr"])          # (storage differences of 1e-11 over a sink of litres)


def test_catchment_c2_f20(product, oracle):
    """C2: 64x64x10 tilted plane, 20 mm in hour 0 (infiltration regime), 6 h."""
    m = cm.catchment_model(64, 64, 10)
    steps = []
    for h, g, o, gd, od in run_pair(product, oracle, m, "F20", 6):
        assert len(gd) == len(od), f"hour {h}: accepted steps {len(gd)} vs {len(od)}"
        np.testing.assert_allclose(gd, od, rtol=1e-12)
        assert_snapshot_close(g, o, f"C2 F20 h{h}")
        steps.append(len(gd))
    assert steps == [22, 13, 6, 3, 3, 3]          # SURVEY.md 8c anchors
    gc, oc = product.counters(), oracle.counters()
    for k in ("attempts", "accepted", "approximations", "courant_rejections", "restores"):
        assert gc[k] == oc[k], (k, gc, oc)


def test_catchment_c2_f60_runoff_regime(product, oracle):
    """C2 with 60 mm in hour 0: hour 0 (76 steps with Courant rejections) and the first 400
    steps of hour 1, where dt is pinned at dtmin and every step ends through restoreBestStep."""
    m = cm.catchment_model(64, 64, 10)
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=1)
    res = []
    for sf in (product, oracle):
        n0, d0 = cm.run_hour(sf, m, 60.0)
        s0 = cm.snapshot(sf, m)
        n1, d1 = cm.run_hour(sf, m, 0.0, max_steps=400)
        res.append((n0, d0, s0, d1, cm.snapshot(sf, m), sf.counters()))
    (gn0, gd0, gs0, gd1, gs1, gc), (on0, od0, os0, od1, os1, oc) = res
    assert gn0 == on0 == 76
    np.testing.assert_allclose(gd0, od0, rtol=1e-12)
    assert_snapshot_close(gs0, os0, "C2 F60 h0")
    np.testing.assert_allclose(gd1, od1, rtol=1e-12)
    assert_snapshot_close(gs1, os1, "C2 F60 h1[:400]")
    assert gc["restores"] == oc["restores"] and gc["restores"] > 300
    assert gc["courant_rejections"] == oc["courant_rejections"] > 0


def test_heterogeneous_soils(product, oracle):
    """12 USDA classes in 8x8 patches (SURVEY.md 8d heterogeneous variant), small grid, 2 h."""
    m = cm.catchment_model(32, 32, 6, heterogeneous=True)
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=1)
    for sf in (product, oracle):
        cm.run_hour(sf, m, 20.0)
    g, o = cm.snapshot(product, m), cm.snapshot(oracle, m)
    assert_snapshot_close(g, o, "het h0")
    for sf in (product, oracle):
        cm.run_hour(sf, m, 0.0, max_steps=300)
    g, o = cm.snapshot(product, m), cm.snapshot(oracle, m)
    assert_snapshot_close(g, o, "het h1[:300]")


def test_getters_and_state_setters_roundtrip(product, oracle):
    """Per-node getters after device steps, and state setters between steps (hourly sinks,
    daily pond, re-imposed potentials) reach the device."""
    m = cm.catchment_model(16, 16, 5)
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=1)
        cm.run_hour(sf, m, 20.0)
        # mid-run edits through the scalar API
        sf.check(sf.lib.sf3d_set_node_matric_potential(m.ns + 5, -1.0), "set psi")
        sf.check(sf.lib.sf3d_set_node_pond(3, 0.004), "set pond")
        sf.check(sf.lib.sf3d_set_node_water_sink_source(m.ns + 40, -1e-7), "set sink")
        sf.lib.sf3d_compute_step(600.0)
    for i in (0, 3, m.ns + 5, m.ns + 40, m.n - 1):
        for fn in ("get_node_total_potential", "get_node_matric_potential", "get_node_water_content",
                   "get_node_degree_of_saturation", "get_node_water_conductivity"):
            a, b = getattr(product, fn)(i), getattr(oracle, fn)(i)
            assert abs(a - b) <= RTOL * max(abs(b), 1e-9), (fn, i, a, b)
    a = product.boundary_water_flow(0, m.n); b = oracle.boundary_water_flow(0, m.n)
    assert rel(a, b, floor=1e-6) < 10 * RTOL
    assert abs(product.get_total_water_content() - oracle.get_total_water_content()) < RTOL * oracle.get_total_water_content()


def test_v1_alias_layer_runs_the_column(product):
    """the retired v1 names (initializeFluxes, setNode(..., isBoundary, v1 boundary codes), computeStep)
    drive the same device path: C1 column, 2 h, against the reference's golden values"""
    import re
    import subprocess
    from pathlib import Path
    from criteria3d_amd import build
    build.build_v1_alias()
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([str(root / "shim" / "v1_alias_demo")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    gold = np.load(root / "tests" / "golden" / "c1_column.npz")
    lines = [l for l in out.stdout.splitlines() if l.startswith("h")]
    assert len(lines) == 2
    for h, line in enumerate(lines):
        v = dict(re.findall(r"(\w+)=([-+0-9.eE]+)", line))
        assert int(v["steps"]) == gold["steps_per_hour"][h]
        assert abs(float(v["storage"]) - gold["storage"][h]) <= 1e-6 * gold["storage"][h]
        assert abs(float(v["drain"]) - gold["drainage"][h]) <= 1e-6 * max(abs(gold["drainage"][h]), 1e-3)
    assert abs(float(dict(re.findall(r"(\w+)=([-+0-9.eE]+)", lines[0]))["H1"]) - gold["H_h0"][1]) <= 1e-6 * abs(gold["H_h0"][1])


def test_irregular_catchment_midsize(product, oracle):
    """~45 k nodes with DEM holes, columns of different depth, three soils and a prescribed-potential
    node: most chunks have no uniform link pattern, so the per-node index path carries the load."""
    m = cm.ragged_model(96, 80, 8)
    assert m.n > 40000
    for sf in (product, oracle):
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, m, threads=8)
        sf.check(sf.lib.sf3d_set_node_prescribed_total_potential(m.meta["prescribed_node"], m.meta["prescribed_H"]), "prescribed")
    res = []
    for sf in (product, oracle):
        n0, d0 = cm.run_hour(sf, m, 30.0)
        s0 = cm.snapshot(sf, m)
        n1, d1 = cm.run_hour(sf, m, 0.0, max_steps=250)
        res.append((d0, s0, d1, cm.snapshot(sf, m), sf.counters()))
    (gd0, gs0, gd1, gs1, gc), (od0, os0, od1, os1, oc) = res
    np.testing.assert_allclose(gd0, od0, rtol=1e-12)
    np.testing.assert_allclose(gd1, od1, rtol=1e-12)
    assert_snapshot_close(gs0, os0, "irregular h0")
    assert_snapshot_close(gs1, os1, "irregular h1")
    for k in ("attempts", "accepted", "approximations", "sweeps", "courant_rejections", "restores"):
        assert gc[k] == oc[k], (k, gc, oc)


def test_reinitialise_and_clean_cycles(product, oracle):
    """initializeSF3D on a live model cleans first (soilFluxes3D.cpp:53); device memory is released
    and rebuilt; a different model after a clean gives the same answer as in a fresh library."""
    ref = None
    for cycle in range(3):
        for mdl, mm in ((cm.catchment_model(16, 16, 4), 20.0), (cm.column_model(50), 5.0)):
            product.check(product.lib.sf3d_reset_solver_state(), "reset")
            cm.build(product, mdl)
            cm.run_hour(product, mdl, mm)
            H = product.total_potential(0, mdl.n)
            if mdl.meta.get("kind") == "column":
                if ref is None:
                    ref = H
                assert np.array_equal(H, ref)
        assert product.lib.sf3d_clean() == capi.OK
        assert product.lib.sf3d_clean() == capi.OK          # idempotent (cpp:220-221)
        assert product.lib.sf3d_get_node_total_potential(0) == -2222.0


@pytest.mark.parametrize("one_way", [False, True])
def test_early_courant_check_takes_the_same_decisions(product, oracle, one_way):
    """The early Courant check (k_props_surface + k_courant_probe) evaluates every runoff link from ONE of its ends and refuses an
    attempt before the full approximation is computed - forced on before every approximation here: the same accepted steps, the same
    counters and the same state as the oracle under the 60 mm hour (Courant rejections), also where a third of the lateral surface
    links exist in one direction only (the end that has the link must then be the one that evaluates it)."""
    import dataclasses
    from tests.scenarios import env
    m = cm.catchment_model(48, 40, 5)
    if one_way:
        rng = np.random.RandomState(3)
        lateral_surface = (m.link_dir == capi.LINK_LATERAL) & (m.link_node < m.ns)
        drop = lateral_surface & (rng.rand(m.link_node.size) < 0.33) & ((m.link_node > m.link_to) == (rng.rand(m.link_node.size) < 0.5))
        keep = ~drop
        m = dataclasses.replace(m, link_node=m.link_node[keep], link_to=m.link_to[keep], link_dir=m.link_dir[keep], link_area=m.link_area[keep])
    with env(SF3D_COURANT_PROBE="always"):
        for sf in (product, oracle):
            sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
            cm.build(sf, m, threads=8)
    # (with one-way links the system loses its symmetry and the run crawls at the minimum dt after its first 100 steps: 150 are taken)
    for mm, mx in (((60.0, 150),) if one_way else ((60.0, None), (0.0, 40))):
        _, gd = cm.run_hour(product, m, mm, max_steps=mx)
        _, od = cm.run_hour(oracle, m, mm, max_steps=mx)
        np.testing.assert_allclose(gd, od, rtol=1e-12)
    g, o = cm.snapshot(product, m), cm.snapshot(oracle, m)
    assert np.max(np.abs(g["H"] - o["H"]) / np.maximum(np.abs(o["H"]), 1e-9)) < 1e-9
    gc, oc = product.counters(), oracle.counters()
    for k in ("attempts", "accepted", "approximations", "sweeps", "courant_rejections", "linear_failures", "restores"):
        assert gc[k] == oc[k], (k, gc, oc)
    assert gc["courant_rejections"] >= (5 if one_way else 30) and gc["early_courant_rejections"] == gc["courant_rejections"], gc
    oracle.lib.sf3d_clean(); product.lib.sf3d_clean()


@pytest.mark.parametrize("seed", list(range(1, 21)))
def test_random_irregular_models_with_every_fast_path_forced(product, oracle, seed):
    """Fuzz over graph shapes: random holes, column depths, layer thicknesses, soils, boundary types and a random subset of the lateral
    links (catchment.random_model), with the fast paths a small grid would not get by itself forced on - the masked paired sweep and the
    early Courant check before every approximation - against the oracle: accepted dt, counters, H and Se after a 30 mm burst and a dry
    stretch."""
    from tests.scenarios import env
    rng = np.random.RandomState(100 + seed)
    m = cm.random_model(seed, nx=int(rng.randint(66, 90)), ny=int(rng.randint(8, 30)), nz=int(rng.randint(3, 7)))
    assert m.ns >= 64
    with env(SF3D_PAIR_SWEEP="1", SF3D_PAIR_W="6", SF3D_COURANT_PROBE="always"):
        for sf in (product, oracle):
            sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
            cm.build(sf, m, threads=4)
    product.check(product.lib.sf3d_kernel_timing(1), "timing")
    for mm, mx in ((30.0, 60), (0.0, 40)):
        _, gd = cm.run_hour(product, m, mm, max_steps=mx)
        _, od = cm.run_hour(oracle, m, mm, max_steps=mx)
        np.testing.assert_allclose(gd, od, rtol=1e-12)
    stats = product.kernel_stats()
    product.lib.sf3d_kernel_timing(0)
    assert stats["k_sweep_pair"][0] > 0, stats          # the masked paired sweep really ran
    g, o = cm.snapshot(product, m), cm.snapshot(oracle, m)
    assert np.max(np.abs(g["H"] - o["H"]) / np.maximum(np.abs(o["H"]), 1e-9)) < 1e-8
    assert np.max(np.abs(g["Se"] - o["Se"])) < 1e-7
    gc, oc = product.counters(), oracle.counters()
    for k in ("attempts", "accepted", "approximations", "sweeps", "courant_rejections", "linear_failures", "restores"):
        assert gc[k] == oc[k], (k, gc, oc)
    oracle.lib.sf3d_clean(); product.lib.sf3d_clean()


def test_every_entry_of_the_paired_pass_kernel_table_gives_the_bits_of_single_sweeps(product):
    """The step driver picks the paired pass's kernel from a table generated over the patch heights (pair_kernel, sf3d_host_build.inc):
    every single-GPU entry - W = 6, 8, 10, 14 x streaming stores off / on x k_sweep_pair / k_sweep_pair_masked - on one small box, each a
    model of its own with SF3D_PAIR_SWEEP=1.  A 30 mm hour capped at 40 steps under sf3d_kernel_timing(2): the sampled steps launch
    eagerly with events, the others replay graphs.  H, Se, every accepted dt and the work counters must be the bits of the same hour
    with SF3D_PAIR_SWEEP=0, and the pass must really have run in all sixteen.
    The box is 64 x 14 x 3: 14 rows are the fewest at which plan_pair_patches accepts W = 14 when asked (it wants NY >= W; held on the
    CPU by calling it for 64 x 13 / 14 / 16 x 3 boxes, full and masked: bestW = 0 at 13 rows, 14 at 14 and 16), and at 14 rows the last
    patch of every height is a short one (4 + 4 + 4 + 2, 6 + 6 + 2, 8 + 6, 12 + 2 owned rows)."""
    from tests.scenarios import env
    m = cm.catchment_model(64, 14, 3)

    def hour(**switches):
        with env(**switches):
            product.check(product.lib.sf3d_reset_solver_state(), "reset")
            cm.build(product, m, threads=4)
            product.check(product.lib.sf3d_kernel_timing(2), "timing")
            _, dts = cm.run_hour(product, m, 30.0, max_steps=40)
            stats = product.kernel_stats()
            product.lib.sf3d_kernel_timing(0)
            out = (np.array(dts), cm.snapshot(product, m), product.counters(), stats)
            product.lib.sf3d_clean()
        return out

    rd, rs, rc, rstats = hour(SF3D_PAIR_SWEEP="0")
    assert len(rd) == 40 or rd.sum() >= 3600.0
    assert rstats["k_sweep_pair"][0] == 0, rstats
    for W in (6, 8, 10, 14):
        for nt in ("0", "1"):
            for masked in (False, True):
                mode = dict(SF3D_PAIR_SWEEP="1", SF3D_PAIR_W=str(W), SF3D_NT_STREAM=nt, **({"SF3D_PAIR_FORCE_MASKED": "1"} if masked else {}))
                gd, gs, gc, stats = hour(**mode)
                assert stats["k_sweep_pair"][0] > 0, (mode, stats)          # no falling back to single sweeps
                assert np.array_equal(gd, rd), mode
                assert np.array_equal(gs["H"], rs["H"]) and np.array_equal(gs["Se"], rs["Se"]), mode
                assert gc == rc, (mode, gc, rc)


def test_sf3d_devices_picks_the_gpu_of_an_unmodified_caller():
    """SF3D_DEVICES: which GPU a caller that never calls sf3d_set_device runs on - entry LOCAL_RANK of the list; a device
    that does not exist is a SolverError at the first device call, not a silent device 0"""
    import os
    import subprocess
    import sys
    code = ("from criteria3d_amd import capi, catchment as cm\n"
            "sf = capi.load_product(); m = cm.column_model()\n"
            "sf.check(sf.lib.sf3d_reset_solver_state(), 'reset')\n"
            "try:\n    cm.build(sf, m)\n    print('built', sf.lib.sf3d_compute_step(60.0) > 0)\nexcept capi.SF3DError as e:\n    print('refused', e)\n")
    ok = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, SF3D_DEVICES="0,0", LOCAL_RANK="1"), timeout=300)
    assert "built True" in ok.stdout, ok.stdout + ok.stderr
    bad = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, SF3D_DEVICES="0,97", LOCAL_RANK="1"), timeout=300)
    assert "refused" in bad.stdout and "SF3D_DEVICES names device 97" in (bad.stdout + bad.stderr), bad.stdout + bad.stderr
