"""What tests/test_localdetrend_host.py, tests/test_gpu_localdetrend.py, tests/golden/make_localdetrend.py and
scripts/multirank_localdetrend_worker.py share (no tests here): the pin tests/golden/localdetrend.npz decoded into its two rasters with
their cases and recorded outcomes; the file format of the host build of the per-cell text (tests/localdetrend_host.cpp), which the pin's
driver reads and writes too; the calls of a case through the binding and through the restatement; and, away from the pin, `synthetic`
with the table OFF_PIN of its arguments: selected lists of exactly 1, 4, 5, 63, 64, 65, 128 and 129 stations, ring-selected lists of 122
to 131 with the full first-guess lists (16, 30 and the 31 of POSITION_31), the arms the pin has below a wave only, and rasters of one
block, a block and a wave, and two blocks.  HOST_ONLY names the cases the restatement is too slow for."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import localdetrend as ld, meteo

ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "localdetrend.npz"
RASTERS = ("relief", "tiny")
PORT = 29801                                    # the two-rank test's (clear of tests/ranks.py's table and of the other blocks' ports)
# the rule of tests/raster_helpers.py same for every recorded quantity: the parameters as raw 64-bit patterns, a NaN in R2 equal to any NaN
QUANTITIES = dict(value="bits", count="value", radius="bits", significant="value", r2="nan", parameters="bits")


def load_pin():
    z = np.load(PIN)
    p = {k: z[k] for k in z.files}
    out = dict(flag=np.float32(p["flag"]), arms=dict(zip((str(n) for n in p["arm_names"]), (int(c) for c in p["arm_counts"]))),
               ranges=json.loads(str(p["ranges"])), cpu=json.loads(str(p["cpu"])))
    for name in RASTERS:
        geo = p[f"{name}_geo"]
        r = dict(name=name, dem=p[f"{name}_dem"], xll=float(geo[0]), yll=float(geo[1]), cell_size=float(geo[2]), flag=out["flag"], cases=[])
        for k, c in enumerate(json.loads(str(p[f"{name}_cases"]))):
            g = lambda key: p[f"{name}_c{k}_{key}"]
            n_par = len(c["fit"]["min"])
            par = np.full(r["dem"].shape + (ld.MAX_PARAMETERS,), ld.NODATA, np.float64)
            par[..., :n_par] = g("par")
            c.update(x=g("x"), y=g("y"), height=g("h"), value=g("v"), area=np.float32(c["area"]),
                     want=dict(value=g("map"), count=g("count").astype(np.uint32), radius=g("radius"), significant=g("sig").astype(bool), r2=g("r2"), parameters=par))
            r["cases"].append(c)
        out[name] = r
    return out


def case_name(c) -> str:
    return f"{c['label']}-{meteo.VARIABLES[c['var']]}-{meteo.METHODS[c['method']]}-{ld.FUNCTIONS[c['fit']['function']]}-min{c['fit']['minPointsLocalDetrending']}"


def settings_of(c) -> dict:
    return ld.local_settings(dict(useDetrending=c["useDetrending"]))


def restated(r, c, mine=None, arms=None) -> dict:
    return ld.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], c["var"], c["method"], c["x"], c["y"], c["height"], c["value"], c["area"], c["fit"],
                                  settings_of(c), float(r["flag"]), mine, arms)


def initialize(sf, r) -> None:
    meteo.initialize(sf, r["dem"], r["xll"], r["yll"], r["cell_size"], [None], float(r["flag"]))


def interpolate(sf, c, download=True):
    return ld.interpolate(sf, c["var"], c["method"], c["x"], c["y"], c["height"], c["value"], c["area"], c["fit"], settings_of(c), download)


def outcome(sf, value) -> dict:
    """the map with what the getters return of the last call, by the names of QUANTITIES"""
    return dict(value=value, **ld.get_selection(sf), **ld.get_fit(sf))


# the first-guess positions of tests/golden/localdetrend.npz's `ranges` whose list has MAX_FIRST_GUESS combinations (position 0 in the
# first two slots: fifteen steps up from the minimum for each of the two walked parameters); tests/test_localdetrend_host.py holds them
# to the pin's record
POSITION_31 = {ld.PIECEWISE_THREE: [0, 0, 0, 1, 1], ld.PIECEWISE_THREE_FREE: [0, 0, 0, 1, 1, 1]}


def synthetic(n_stations: int, min_points_local: int, method: int, function: int = ld.PIECEWISE_TWO, guesses: int | None = 2, seed: int = 7,
              var: int = meteo.AIR_TEMPERATURE, use_detrending: int = 1, std_dev_threshold: float = ld.NODATA, equal: bool = False, shape: tuple = (3, 11),
              flag_cell: tuple = (1, 5), position=None, vee: bool = False, points_range=None, low_guess=None) -> tuple:
    """(raster, case) away from the pin: `shape` cells of 500 m (3 x 11: 33 cells, a partial last block of four) with one flag cell and
    `n_stations` stations up to 20 km around it, none twice at one place; the first `guesses` combinations (None: all) of the default range
    walked from `position` (None: the minimum of parameter 0, the middle of the others).  equal: every station holds one value; vee: the
    values fall to 900 m and rise above it, which the first guess fits badly; points_range: in the place of the values' own; low_guess:
    (k, j, value) puts parameter j of first guess k there - below the range, every step is clamped back and the iteration cap ends the fit"""
    rng = np.random.default_rng(seed + n_stations)
    (rows, cols), cs, xll, yll = shape, 500.0, 512000.0, 4870000.0
    r_, c_ = np.mgrid[0:rows, 0:cols]
    dem = np.round(200.0 + 70.0 * c_ - 40.0 * r_, 1).astype(np.float32)
    dem[flag_cell] = np.float32(-9999.0)
    x = np.round(xll + rng.uniform(-20000.0, cols * cs + 20000.0, n_stations), 2)
    y = np.round(yll + rng.uniform(-20000.0, rows * cs + 20000.0, n_stations), 2)
    h = np.round(rng.uniform(20.0, 1900.0, n_stations), 1).astype(np.float32)
    t = np.round(np.where(h < 350.0, 9.0 + 0.006 * h, 11.1 - 0.0055 * (h - 350.0)) + rng.normal(0.0, 0.6, n_stations), 1).astype(np.float32)
    if equal:
        t[:] = np.float32(11.5)
    if vee:
        t = np.round(6.0 + 0.012 * np.abs(h - 900.0) + rng.normal(0.0, 0.3, n_stations), 1).astype(np.float32)
    n = ld.PARAMETERS[function]
    configured = {ld.PIECEWISE_TWO: [0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 0.007, -0.0015],
                  ld.PIECEWISE_THREE: [-350.0, 0.0, 0.0, 0.002, -0.01, 2500.0, 0.0, 1000.0, 0.007, -0.0015],
                  ld.PIECEWISE_THREE_FREE: [-350.0, 0.0, 0.0, 0.002, -0.01, -0.01, 2500.0, 0.0, 1000.0, 0.007, -0.0015, -0.0015]}[function]
    fit = ld.make_fit(function, configured, [0] + [1] * (n - 1) if position is None else list(position),
                      (float(t.min()), float(t.max())) if points_range is None else points_range, min_points_local, std_dev_threshold)
    fit["first_guess"] = [list(g) for g in fit["first_guess"][:guesses]]
    if low_guess is not None:
        fit["first_guess"][low_guess[0]][low_guess[1]] = float(low_guess[2])
    area = np.float32((np.float32(x.max()) - np.float32(x.min())) * (np.float32(y.max()) - np.float32(y.min())))
    r = dict(name=f"synthetic{n_stations}", dem=dem, xll=xll, yll=yll, cell_size=cs, flag=np.float32(-9999.0))
    c = dict(label="synthetic", var=var, method=method, fit=fit, useDetrending=use_detrending, x=x, y=y, height=h, value=t, area=area)
    return r, c


def _off_pin() -> tuple:
    """(label, the arguments of `synthetic` by name)"""
    I, S, M = meteo.IDW, meteo.SHEPARD, meteo.SHEPARD_MODIFIED
    T2, T3F, T3 = ld.PIECEWISE_TWO, ld.PIECEWISE_THREE_FREE, ld.PIECEWISE_THREE
    out = []
    # the wave's edges: every station selected, so every cell's list has exactly n entries - less than the validity minimum, at it, a full
    # ballot less one, full, one spilt, two full, a third of one entry
    for n, mpl in ((1, 5), (4, 5), (5, 4), (63, 60), (64, 60), (65, 60), (128, 110), (129, 110)):
        for method in (I, S, M):
            out.append((f"edge{n}-{meteo.METHODS[method]}", dict(n_stations=n, min_points_local=mpl, method=method, function=T3F, guesses=3)))
    # long lists from rings, the full first-guess lists: 30 and 31 busy fit lanes
    out.append(("rings150-three-30", dict(n_stations=150, min_points_local=60, method=M, function=T3, guesses=None)))
    out.append(("rings150-free-31", dict(n_stations=150, min_points_local=60, method=S, function=T3F, guesses=None, position=POSITION_31[T3F])))
    out.append(("rings150-two-16", dict(n_stations=150, min_points_local=60, method=I, function=T2, guesses=None)))
    out.append(("all70-three-30", dict(n_stations=70, min_points_local=60, method=M, function=T3, guesses=None)))
    # arms the pin has below a wave only
    out.append(("dew70-undetrended", dict(n_stations=70, min_points_local=60, method=I, function=T3F, guesses=3, var=meteo.AIR_DEW_TEMPERATURE, use_detrending=0)))
    out.append(("equal70", dict(n_stations=70, min_points_local=60, method=M, function=T3, guesses=4, equal=True)))
    # the iteration cap (1 000 iterations a fit: the restatement takes 0.6 s a cell, hence five cells) and a later guess taking over
    out.append(("cap70", dict(n_stations=70, min_points_local=60, method=I, function=T2, guesses=3, points_range=(16.0, 25.0), low_guess=(1, 1, 10.5),
                              shape=(1, 5), flag_cell=(0, 3))))
    out.append(("vee150-free-30", dict(n_stations=150, min_points_local=60, method=M, function=T3F, guesses=None, vee=True)))
    # a threshold above the heights' deviation: no fit, 70 stations interpolated undetrended
    out.append(("flat70", dict(n_stations=70, min_points_local=60, method=S, function=T2, guesses=2, std_dev_threshold=5000.0)))
    # block shapes (four waves a block): one block, a second of one wave with the flag in the raster's first cell, two full blocks
    out.append(("block1x4", dict(n_stations=70, min_points_local=60, method=M, function=T3F, guesses=3, shape=(1, 4), flag_cell=(0, 2))))
    out.append(("block1x5", dict(n_stations=70, min_points_local=60, method=I, function=T3F, guesses=3, shape=(1, 5), flag_cell=(0, 0))))
    out.append(("block2x4", dict(n_stations=70, min_points_local=60, method=M, function=T3, guesses=3, shape=(2, 4), flag_cell=(1, 0))))
    return tuple(out)


OFF_PIN = _off_pin()
# the full lists of the three-piece functions: the restatement takes 10 to 30 s a case, so they are held host build against device only
HOST_ONLY = ("rings150-three-30", "rings150-free-31", "vee150-free-30", "all70-three-30")


def off_pin(label: str) -> tuple:
    r, c = synthetic(**dict(OFF_PIN)[label])
    r["name"], c["label"] = label, label
    return r, c


def ties(r, c) -> bool:
    """two stations of a cell's selected list at one float distance (shepardIdw's std::sort leaves their order open)"""
    cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
    for row, col in np.argwhere(r["dem"] != r["flag"]):
        _, d, _, _ = ld.local_selection(cx[row, col], cy[row, col], c["x"], c["y"], c["fit"]["minPointsLocalDetrending"], c["area"])
        if d is None:
            dx, dy = np.asarray(c["x"]).astype(np.float32) - np.float32(cx[row, col]), np.asarray(c["y"]).astype(np.float32) - np.float32(cy[row, col])
            d = np.sqrt(dx * dx + dy * dy)
        if len(set(np.asarray(d).tolist())) != len(d):
            return True
    return False


# ---- the file format of tests/localdetrend_host.cpp (its header comment)

def fit_table(fit: dict) -> np.ndarray:
    t = np.zeros((3 + ld.MAX_FIRST_GUESS, ld.MAX_PARAMETERS), np.float64)
    n = len(fit["min"])
    t[0, :n], t[1, :n], t[2, :n] = fit["min"], fit["max"], fit["delta"]
    for k, g in enumerate(fit["first_guess"]):
        t[3 + k, :n] = g[:n]
    return t


def case_head(c) -> np.ndarray:
    fit = c["fit"]
    return np.array([c["var"], c["method"], fit["function"], len(fit["min"]), len(fit["first_guess"]), fit["minPointsLocalDetrending"], c["useDetrending"], len(c["x"])], np.int32)


def input_parts(r, cases) -> list:
    parts = [np.array([r["dem"].shape[0], r["dem"].shape[1], len(cases)], np.int32), np.array([r["flag"]], np.float32),
             np.array([r["xll"], r["yll"], r["cell_size"]], np.float64), r["dem"].astype(np.float32)]
    for c in cases:
        parts += [case_head(c), np.array([c["fit"]["stdDevThreshold"], c["area"]], np.float32), fit_table(c["fit"])]
        parts += [np.asarray(a, t) for a, t in ((c["x"], np.float64), (c["y"], np.float64), (c["height"], np.float32), (c["value"], np.float32))]
    return parts


def output_of(raw: bytes, r, cases) -> list:
    from tests.raster_helpers import Reader
    shape, out, o = r["dem"].shape, Reader(raw), []
    for _ in cases:
        o.append(dict(value=out.take(np.float32, *shape), count=out.take(np.uint32, *shape), radius=out.take(np.float32, *shape),
                      significant=out.take(np.int32, *shape).astype(bool), r2=out.take(np.float32, *shape), parameters=out.take(np.float64, *shape, ld.MAX_PARAMETERS)))
    assert out.done()
    return o


def write_input(path, r, cases) -> None:
    """for the pin's driver (tests/golden/make_localdetrend.py), which reads and writes the program's format"""
    from tests.raster_helpers import write_parts
    write_parts(path, input_parts(r, cases))


def read_output(path, r, cases) -> list:
    return output_of(Path(path).read_bytes(), r, cases)


def run_host(exe, r, directory, cases=None) -> list:
    """the host program on one raster -> the outcome of every case"""
    from tests.raster_helpers import run_host_program
    cases = r["cases"] if cases is None else cases
    return output_of(run_host_program(exe, directory, r["name"], input_parts(r, cases)), r, cases)
