"""Link flow sums added in batches (k_links_flush: the sums of up to SF3D_LINKS_RING accepted steps in one pass) against the
per-step form (SF3D_OVERLAP_ACCEPT=0: k_accept inside every step), bit for bit.

Every case runs the same model and forcing twice in one process, once per form, through the same calls; what both runs read - the link
flow sums through the reference's getters (up, down, and maximum / sum / inflow / outflow of the eight laterals: together all ten slots of a
node), the boundary sums, H, Se and the accepted time steps - must be equal arrays.  The grids are the smallest on which the kernel's
index forms all occur: 5 x 7 x 3 (105 nodes: no full chunk of 64), 20 x 13 x 4 (260 surface nodes: a chunk holding surface and soil rows,
row ends), the ragged graph (per-node link tables) and the Urban / Road catchment."""
import numpy as np
import pytest

from criteria3d_amd import catchment as cm, maps
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

R = 8          # SF3D_LINKS_RING of the default build (sf3d_device.h)


class Run:
    """the caller's hourly loop (catchment.run_hour), cut into single computeStep calls so that a case can act between any two steps"""

    def __init__(self, sf, m, sinks):
        self.sf, self.m, self.sinks = sf, m, sinks
        self.hour, self.t, self.dts = -1, 3600.0, []

    def next_hour(self):
        self.hour += 1; self.t = 0.0
        self.sf.set_sink_source_bulk(0, self.sinks(self.hour, self.m))

    def steps(self, n):
        for _ in range(n):
            if self.t >= 3600.0:
                self.next_hour()
            dt = self.sf.lib.sf3d_compute_step(3600.0 - self.t)
            assert dt > 0.0, dt
            self.dts.append(dt); self.t += dt

    def rest_of_hour(self):
        while self.t < 3600.0:
            self.steps(1)

    def read(self, out, tag):
        sf, m = self.sf, self.m
        out[tag + ":flows"] = cm.link_flows(sf, m)
        out[tag + ":boundary"] = sf.boundary_water_flow(0, m.n)
        out[tag + ":H"] = sf.total_potential(0, m.n)
        out[tag + ":Se"] = sf.degree_of_saturation(0, m.n)
        out[tag + ":dts"] = np.array(self.dts)


def _rain(first_hour_mm):
    return lambda h, m: np.full(m.ns, cm.rain_rate(first_hour_mm if h == 0 else 0.0, m.cell_area))


MODELS = {
    "5x7x3": (lambda: cm.catchment_model(5, 7, 3), _rain(20.0), None),
    "20x13x4": (lambda: cm.catchment_model(20, 13, 4), _rain(20.0), None),
    "flows_ragged": (cm.ragged_model, sc._ragged_sinks, sc._ragged_pre),
    "urban_road": (cm.urban_road_model, _rain(30.0), None),
    "c2": (lambda: cm.catchment_model(64, 64, 10), _rain(60.0), None),
}


def _both_forms(product, model, script):
    """script(run, out) on a fresh model, once with the sums in batches and once per step -> the two dicts of what it read"""
    res = []
    for form in ("1", "0"):
        make, sinks, pre = MODELS[model]
        m = make()
        with sc.env(SF3D_OVERLAP_ACCEPT=form):
            product.check(product.lib.sf3d_reset_solver_state(), "reset")
            cm.build(product, m, threads=1)
            if pre is not None:
                pre(product, m)
            out = {}
            script(Run(product, m, sinks), out)
            out["counters"] = product.counters()
            product.lib.sf3d_clean()
        res.append(out)
    return res


def _assert_same(ring, step):
    assert ring.keys() == step.keys()
    for k in ring:
        if k == "counters":
            assert ring[k] == step[k], (ring[k], step[k])
        else:
            assert np.array_equal(ring[k], step[k]), f"{k}: {int(np.sum(ring[k] != step[k]))} of {ring[k].size} values differ from the per-step form"


@pytest.mark.parametrize("n", [1, R - 1, R, R + 1, 2 * R + 3])
@pytest.mark.parametrize("model", ["5x7x3", "20x13x4", "flows_ragged", "urban_road"])
def test_sums_of_n_steps_equal_the_per_step_sums_bitwise(product, model, n):
    """n accepted steps without anything in between: a partly filled ring, a full one, one that was emptied once and twice"""
    def script(run, out):
        run.steps(n)
        run.read(out, f"after {n}")
    ring, step = _both_forms(product, model, script)
    assert len(ring[f"after {n}:dts"]) == n
    assert np.any(ring[f"after {n}:flows"] != 0.0)
    _assert_same(ring, step)


def test_refused_attempts_and_restored_steps_keep_the_sums_bitwise(product):
    """C2 F60 (64 x 64 x 10 under 60 mm) cut the way the scenario plans of tests/scenarios.py cut an hour: the first 40 accepted steps of hour 0
    (Courant refusals re-assemble a step's slot of the ring), then 25 steps under the forcing of hour 1 (the oracle counts 31 refusals and 8
    restoreBestStep calls in these 65 steps, the first restored step being the 9th of hour 1)"""
    def script(run, out):
        run.steps(40)
        run.read(out, "hour 0, 40 steps")
        run.t = 3600.0                      # (max_steps of catchment.run_hour: the caller goes on to the next hour's forcing)
        run.steps(25)
        assert run.hour == 1
        run.read(out, "hour 1, 25 steps")
    ring, step = _both_forms(product, "c2", script)
    assert ring["counters"]["restores"] > 0 and ring["counters"]["courant_rejections"] > 0, ring["counters"]
    _assert_same(ring, step)


def _getter(run, out):
    run.steps(3); run.read(out, "after 3"); run.steps(3); run.read(out, "after 6")


def _synchronize(run, out):
    run.steps(3)
    run.sf.check(run.sf.lib.sf3d_synchronize(), "synchronize")
    run.steps(3); run.read(out, "after 6")


def _state_setter(run, out):
    """pending sums must be those of the ACCEPTED heads, not of what the setter puts in their place"""
    run.steps(3)
    m = run.m
    psi = np.full(m.n, 0.5 * m.psi0_soil); psi[:m.ns] = m.psi0_surface
    run.sf.set_matric_potential_bulk(0, psi)
    run.steps(3); run.read(out, "after 6")


def _initialize_balance(run, out):
    run.steps(3)
    run.sf.check(run.sf.lib.sf3d_initialize_balance(), "initialize_balance")
    out["restart"] = cm.link_flows(run.sf, run.m)
    assert not np.any(out["restart"]), "initializeBalance zeroes the flow sums: nothing pending may be added afterwards"
    run.steps(3); run.read(out, "after 6")


def _timing_mode(run, out):
    """--time-all-kernels steps add their sums inside the step: what is pending comes first"""
    run.steps(3)
    run.sf.check(run.sf.lib.sf3d_kernel_timing(1), "kernel_timing")
    run.steps(2)
    run.sf.check(run.sf.lib.sf3d_kernel_timing(0), "kernel_timing")
    run.steps(2); run.read(out, "after 7")


def _rebuild(run, out):
    """another N while sums are pending: the rings go with the model, nothing of the old one is added to the new one"""
    run.steps(3)
    sf = run.sf
    sf.lib.sf3d_clean()
    m2 = cm.catchment_model(5, 7, 3)
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m2, threads=1)
    run2 = Run(sf, m2, run.sinks)
    run2.steps(3); run2.read(out, "small model after 3")


def _output_map(run, out):
    maps.set_columns(run.sf, *maps.columns(run.m))
    run.steps(3)
    out["inflow map"] = maps.output_maps(run.sf, run.m, maps.WATER_INFLOW)
    out["outflow map"] = maps.output_maps(run.sf, run.m, maps.WATER_OUTFLOW)
    assert np.any(out["inflow map"] > 0.0)
    run.steps(3); run.read(out, "after 6")


@pytest.mark.parametrize("script", [_getter, _synchronize, _state_setter, _initialize_balance, _timing_mode, _rebuild, _output_map],
                         ids=lambda f: f.__name__.strip("_"))
def test_every_flush_point_leaves_the_per_step_sums(product, script):
    ring, step = _both_forms(product, "20x13x4", script)
    _assert_same(ring, step)


def test_device_bytes_count_the_rings(product):
    """the form with the sums in batches really holds the rings: R - 2 more matrices of 80 B per node and R head copies of 8 B per node"""
    m = cm.catchment_model(20, 13, 4)
    got = {}
    for form in ("1", "0"):
        with sc.env(SF3D_OVERLAP_ACCEPT=form):
            product.check(product.lib.sf3d_reset_solver_state(), "reset")
            cm.build(product, m, threads=1)
            Run(product, m, _rain(20.0)).steps(1)
            got[form] = int(product.lib.sf3d_device_bytes())
            product.lib.sf3d_clean()
    assert got["1"] - got["0"] == (R - 2) * 80 * m.n + R * 8 * m.n, got


def test_batched_sums_match_the_oracle(product, oracle):
    """flows_c2_f20 (35 accepted steps in two hours) in the default form against the oracle, with the tolerances of tests/test_gpu_flows.py"""
    from tests.test_gpu_flows import RTOL, flows_close
    with sc.env(SF3D_OVERLAP_ACCEPT="1", SF3D_COMPAT_STALE_LINK_FLOW="0"):
        g = sc.run_scenario(product, "flows_c2_f20")
    o = sc.run_scenario(oracle, "flows_c2_f20")
    np.testing.assert_allclose(g["dts"], o["dts"], rtol=1e-12)
    flows_close(g["link_flows"], o["link_flows"], "flows_c2_f20, sums in batches, vs oracle")
    assert np.max(np.abs(g["boundary_flow"] - o["boundary_flow"])) <= RTOL * max(np.max(np.abs(o["boundary_flow"])), 1e-9)
    product.lib.sf3d_clean(); oracle.lib.sf3d_clean()
