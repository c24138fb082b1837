"""What tests/test_multidetrend_host.py, tests/test_gpu_multidetrend.py, tests/golden/make_multidetrend.py,
scripts/multirank_multidetrend_worker.py and scripts/multidetrend_timing.py share (no tests here): the pin
tests/golden/multidetrend.npz decoded into its two rasters with their proxy rasters, cases, points and recorded outcomes; the file format
of the host build of the kernels' text (tests/multidetrend_host.cpp), which the pin's driver reads and writes too; the calls of a case
through the binding and through the restatement; and, away from the pin, `synthetic` with the table OFF_PIN of its arguments, each row
with the property the host build's outcome must show.

A raster carries SLOTS proxy slots as tests/localproxies_cases.py's do.  A case is a case of localproxies_cases with `points`: None, or
dict(x, y, z: floats; values: [SLOTS, points] floats) - what sf3d_multidetrend_points is called with behind the case's interpolate."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import localdetrend as ld, meteo, multidetrend as md
from tests import localdetrend_cases as lc, localproxies_cases as pc

ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "multidetrend.npz"
RASTERS = ("relief", "tiny")
SLOTS = pc.SLOTS
PORT = 29807                                    # the two-rank test's (clear of tests/ranks.py's table and of the other blocks' ports)
# the rule of tests/raster_helpers.py same for every recorded quantity
QUANTITIES = dict(value="bits", **md.FIT_QUANTITIES, points="bits")
CALL_QUANTITIES = {k: v for k, v in QUANTITIES.items() if k != "points"}
NODATA32 = np.float32(ld.NODATA)

proxies_of = pc.proxies_of
maps_of = pc.maps_of


def case_name(c) -> str:
    active = "".join(str(int(a)) for a in c["active"])
    return f"{c['label']}-{meteo.VARIABLES[c['var']]}-{meteo.METHODS[c['method']]}-{ld.FUNCTIONS[c['fit']['function']]}-{active}"


def load_pin():
    z = np.load(PIN)
    p = {k: z[k] for k in z.files}
    out = dict(flag=np.float32(p["flag"]), arms=dict(zip((str(n) for n in p["arm_names"]), (int(c) for c in p["arm_counts"]))), notes=json.loads(str(p["notes"])))
    for name in RASTERS:
        geo = p[f"{name}_geo"]
        r = dict(name=name, dem=p[f"{name}_dem"], maps=p[f"{name}_maps"], xll=float(geo[0]), yll=float(geo[1]), cell_size=float(geo[2]), flag=out["flag"], cases=[])
        for k, c in enumerate(json.loads(str(p[f"{name}_cases"]))):
            g = lambda key: p[f"{name}_c{k}_{key}"]
            n_par = len(c["fit"]["min"])
            par = np.full(ld.MAX_PARAMETERS, ld.NODATA, np.float64)
            par[:n_par] = g("par")
            c.update(x=g("x"), y=g("y"), proxy_values=g("pv"), value=g("v"), area=np.float32(c["area"]))
            # the pin records the points behind the stations' own
            c["points"] = joined(station_points(c), dict(x=g("px"), y=g("py"), z=g("pz"), values=g("ppv")))
            c.update(want=dict(value=g("map"), significant=bool(g("sig")), r2=np.float32(g("r2")), parameters=par, proxy_significant=g("psig").astype(bool), slope=g("slope"),
                               intercept=g("icpt"), fitted=int(g("fitted")), kept=int(g("kept")), detrended=g("det"), station_kept=g("skept").astype(bool),
                               points=g("pout")))
            r["cases"].append(c)
        out[name] = r
    return out


def restated(r, c, mine=None, arms=None) -> dict:
    """the restatement of a case: the map, the fit's quantities and, where the case has points, their values"""
    out = md.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], maps_of(r), c["var"], c["method"], c["x"], c["y"], c["value"], c["proxy_values"],
                                 c["area"], c["fit"], proxies_of(c), c["others"], dict(useDetrending=c["useDetrending"]), float(r["flag"]), mine, arms)
    if c.get("points") is not None:
        q = c["points"]
        out["points"] = md.restate_points(out["fit"], c["method"], c["x"], c["y"], q["x"], q["y"], q["values"], c["area"], dict(useDetrending=c["useDetrending"]), arms)
    return out


def initialize(sf, r) -> None:
    pc.initialize(sf, r)


def interpolate(sf, c, download=True):
    return md.interpolate(sf, c["var"], c["method"], c["x"], c["y"], c["value"], c["proxy_values"], c["area"], c["fit"], proxies_of(c), c["others"],
                          dict(useDetrending=c["useDetrending"]), download)


def points(sf, c) -> np.ndarray:
    q = c["points"]
    return md.points(sf, q["x"], q["y"], q["z"], q["values"])


def outcome(sf, value, c=None) -> dict:
    """the map with what the getter returns of the last call, by the names of QUANTITIES; c: and the case's points"""
    out = dict(value=value, **md.get_fit(sf))
    if c is not None and c.get("points") is not None:
        out["points"] = points(sf, c)
    return out


# ---- the points of a case

def station_points(c) -> dict:
    """computeResiduals' points: every station at its own float coordinates with its own proxy values, z its height"""
    return dict(x=np.asarray(c["x"], np.float64).astype(np.float32), y=np.asarray(c["y"], np.float64).astype(np.float32), z=np.asarray(c["proxy_values"][0], np.float32),
                values=np.asarray(c["proxy_values"], np.float32).copy())


def joined(a: dict, b: dict) -> dict:
    return dict(x=np.concatenate([a["x"], b["x"]]), y=np.concatenate([a["y"], b["y"]]), z=np.concatenate([a["z"], b["z"]]),
                values=np.concatenate([a["values"], b["values"]], axis=1))


def with_points(r, c, extra=True) -> dict:
    """the case with its points: every station (station_points), and where `extra` a cell centre, a point outside the raster and a cell
    centre whose every proxy value is NODATA - the last three with getProxyValuesXY's values (md.proxy_values_xy)"""
    q = station_points(c)
    if extra:
        rows, cols = r["dem"].shape
        cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
        inside = np.argwhere(r["dem"] != r["flag"])
        a, b = inside[len(inside) // 2], inside[-1]
        ex = np.array([cx[a[0], a[1]], r["xll"] - 3.3 * r["cell_size"], cx[b[0], b[1]]], np.float32)
        ey = np.array([cy[a[0], a[1]], r["yll"] + (rows + 2.4) * r["cell_size"], cy[b[0], b[1]]], np.float32)
        ev = md.proxy_values_xy(r["dem"], r["xll"], r["yll"], r["cell_size"], maps_of(r), proxies_of(c), ex, ey, float(r["flag"]))
        ev[:, 2] = NODATA32                                                     # a point that lacks every proxy: the significant ones among them
        ez = np.array([r["dem"][a[0], a[1]], NODATA32, r["dem"][b[0], b[1]]], np.float32)
        q = joined(q, dict(x=ex, y=ey, z=ez, values=ev))
    return dict(c, points=q)


def cut_points(c, n: int) -> dict:
    """the case with `n` points: its own repeated and cut"""
    q = c["points"]
    take = np.arange(n) % len(q["x"])
    return dict(c, points=dict(x=q["x"][take], y=q["y"][take], z=q["z"][take], values=q["values"][:, take]))


# ---- away from the pin

def synthetic(n_stations: int, method: int, n_others: int, function: int = ld.PIECEWISE_TWO, guesses: int | None = 2, seed: int = 5, position=None,
              use_detrending: int = 1, var: int = meteo.AIR_TEMPERATURE, no_height_every: int | None = None, erase_first: int = 0, keep=None, thresholds=None,
              spoil=None, height_active: bool = True, extra_points: bool = True, shape=None) -> tuple:
    """(raster, case) away from the pin: localproxies_cases.synthetic's 3 x 11 raster, stations and proxies.  position: the first-guess
    positions (None: localdetrend_cases.synthetic's); no_height_every: every k-th station has no height; erase_first: the first stations
    have no value of slot 1, so the prunings erase them where slot 1 passes the first validity pass; keep: a mask or slice over the
    stations, applied last (a sparser hour of the same stations); shape: another raster under the same stations (the same corner and cell
    size, localdetrend_cases.synthetic's plane with its flag cell, proxy rasters of localproxies_cases.synthetic_rasters)"""
    r, c = pc.synthetic(n_stations, 5, method, n_others, seed, function, guesses, height_active=height_active, thresholds=thresholds, spoil=spoil)
    if shape is not None:
        r_, c_ = np.mgrid[0:shape[0], 0:shape[1]]
        r["dem"] = np.round(200.0 + 70.0 * c_ - 40.0 * r_, 1).astype(np.float32)
        r["dem"][1, 5] = r["flag"]
        r["maps"] = pc.synthetic_rasters(shape, np.random.default_rng(seed + 1000))
        r["maps"][2][0, 3] = r["flag"]
    if position is not None:
        c["fit"] = lc.synthetic(n_stations, 5, method, function, guesses, position=position)[1]["fit"]
    c["fit"] = dict(c["fit"], minPointsLocalDetrending=0)
    c["useDetrending"], c["var"] = use_detrending, var
    pv = c["proxy_values"]
    if no_height_every:
        pv[0][::no_height_every] = NODATA32
    if erase_first:
        pv[1][:erase_first] = NODATA32
    if keep is not None:
        c.update(x=c["x"][keep], y=c["y"][keep], value=c["value"][keep], proxy_values=pv[:, keep])
    return r, with_points(r, c, extra_points)


def _full(n):
    def must(r, c, g):
        assert g["status"] == 0 and g["fitted"] == n == len(c["x"]) and g["kept"] <= n and g["station_kept"].sum() == g["kept"]
        assert (g["detrended"][~g["station_kept"]] == NODATA32).all() and (g["detrended"][g["station_kept"]] != NODATA32).all()
    return must


def _four(r, c, g):
    _full(4)(r, c, g)
    assert not g["significant"] and g["r2"] == NODATA32 and (g["parameters"] == ld.NODATA).all() and not g["proxy_significant"].any() and g["kept"] == 4


def _small(n):
    def must(r, c, g):
        _full(n)(r, c, g)
        assert g["significant"] and g["r2"] != NODATA32 and g["kept"] == n
    return must


def _edge(n):
    def must(r, c, g):
        _full(n)(r, c, g)
        assert g["significant"] and g["proxy_significant"][1:3].all() and 0 < n - g["kept"] < n // 4
    return must


def _no_height_third(r, c, g):
    _full(70)(r, c, g)
    h = c["proxy_values"][0]
    assert (h == NODATA32).sum() == 24 and g["significant"]
    # a station without a height is detrended by the function of -9999 and stays in the list
    assert g["station_kept"][h == NODATA32].any()


def _erased_chunk(r, c, g):
    _full(150)(r, c, g)
    assert g["proxy_significant"][1] and not g["station_kept"][:64].any() and g["station_kept"][64:].any()


def _guesses31(function):
    def must(r, c, g):
        _full(40)(r, c, g)
        assert len(c["fit"]["first_guess"]) == 31 and c["fit"]["function"] == function and g["significant"]
    return must


def _kept(n):
    def must(r, c, g):
        _full(n)(r, c, g)
        assert g["kept"] == n and g["significant"]
    return must


def _cells256(r, c, g):
    _full(40)(r, c, g)
    assert r["dem"].size == 256 and g["proxy_significant"][1]


def _no_retrend(r, c, g):
    _full(40)(r, c, g)
    assert c["useDetrending"] == 0 and (g["significant"] or g["proxy_significant"].any())


def _off_pin() -> tuple:
    """(label, the arguments of `synthetic` by name, what the host build's outcome must show)"""
    I, S, M = meteo.IDW, meteo.SHEPARD, meteo.SHEPARD_MODIFIED
    out = [("list4", dict(n_stations=4, method=I, n_others=1), _four), ("list5", dict(n_stations=5, method=S, n_others=0), _small(5)),
           ("list6", dict(n_stations=6, method=M, n_others=0), _small(6))]
    # the wave's edges: the fill, the prunings' ballots and the compaction 64 entries at a time
    out += [(f"list{n}", dict(n_stations=n, method=(I, S, M)[n % 3], n_others=2), _edge(n)) for n in (63, 64, 65, 127, 128, 129)]
    # the cap the LDS arrays and the block's buffers are sized for
    out += [(f"list{n}", dict(n_stations=n, method=I, n_others=2, extra_points=False), _edge(n)) for n in (1023, 1024)]
    out += [
        ("no-height-third", dict(n_stations=70, method=S, n_others=1, no_height_every=3), _no_height_third),
        # the first 64 stations erased by the prunings: the first chunk's ballot of the compaction is 0
        ("erased-chunk", dict(n_stations=150, method=I, n_others=2, erase_first=64), _erased_chunk),
        ("guesses31-three", dict(n_stations=40, method=S, n_others=1, function=ld.PIECEWISE_THREE, guesses=31, position=[0, 0, 1, 1, 1]), _guesses31(ld.PIECEWISE_THREE)),
        ("guesses31-free", dict(n_stations=40, method=I, n_others=0, function=ld.PIECEWISE_THREE_FREE, guesses=31, position=[0, 0, 1, 1, 1, 1]),
         _guesses31(ld.PIECEWISE_THREE_FREE)),
        ("no-retrend-dew", dict(n_stations=40, method=M, n_others=3, use_detrending=0, var=meteo.AIR_DEW_TEMPERATURE), _no_retrend),
        # a raster of exactly 256 cells: one full block of k_multidetrend_cells and no other
        ("cells256", dict(n_stations=40, method=S, n_others=2, shape=(8, 32)), _cells256),
    ]
    # kept lists one below, at and one above the 256 stations a block of k_multidetrend_cells stages in one pass
    out += [(f"kept{n}", dict(n_stations=n, method=(I, S, M)[n % 3], n_others=0, extra_points=False), _kept(n)) for n in (255, 256, 257)]
    return tuple(out)


OFF_PIN = _off_pin()
OFF_PIN_LABELS = tuple(row[0] for row in OFF_PIN)


def off_pin(label: str) -> tuple:
    r, c = synthetic(**{row[0]: row[1] for row in OFF_PIN}[label])
    r["name"], c["label"] = label, label
    return r, c


def must_of(label: str):
    return next(row[2] for row in OFF_PIN if row[0] == label)


def two_hours() -> tuple:
    """(raster, [a full hour, a sparse hour of the same stations]): 129 stations, then every fifth of them - 26, within the first chunk"""
    r, full = synthetic(n_stations=129, method=meteo.IDW, n_others=2)
    _, sparse = synthetic(n_stations=129, method=meteo.IDW, n_others=2, keep=slice(0, None, 5))
    r["name"] = "two-hours"
    full["label"], sparse["label"] = "full", "sparse"
    return r, [full, sparse]


# ---- the file format of tests/multidetrend_host.cpp (its header comment)

def input_parts(r, cases) -> list:
    parts = [np.array([r["dem"].shape[0], r["dem"].shape[1], len(cases)], np.int32), np.array([r["flag"]], np.float32),
             np.array([r["xll"], r["yll"], r["cell_size"]], np.float64), r["dem"].astype(np.float32), np.asarray(r["maps"], np.float32)]
    for c in cases:
        o = dict(useMultipleDetrending=1, useLocalDetrending=0, nProxies=SLOTS, pointsOnly=0, nullArrays=0)
        o.update(c.get("options", {}))
        parts += [lc.case_head(c), np.array([o["useMultipleDetrending"], o["useLocalDetrending"], o["nProxies"], o["pointsOnly"], o["nullArrays"]], np.int32),
                  np.array(c["active"], np.int32), np.array([c["fit"]["stdDevThreshold"], c["area"]], np.float32),
                  np.array([q["stdDevThreshold"] for q in c["others"]], np.float32), np.array([list(q["min"]) + list(q["max"]) for q in c["others"]], np.float64),
                  lc.fit_table(c["fit"]), np.asarray(c["x"], np.float64), np.asarray(c["y"], np.float64), np.asarray(c["proxy_values"], np.float32),
                  np.asarray(c["value"], np.float32)]
        q = c.get("points")
        if q is None:
            parts.append(np.array([-1], np.int32))
        else:
            parts += [np.array([len(q["x"])], np.int32), np.asarray(q["x"], np.float32), np.asarray(q["y"], np.float32), np.asarray(q["z"], np.float32),
                      np.asarray(q["values"], np.float32)]
    return parts


def output_of(raw: bytes, r, cases) -> list:
    """per case dict(status, points_status, and the quantities that follow them)"""
    from tests.raster_helpers import Reader
    shape, out, o = r["dem"].shape, Reader(raw), []
    for c in cases:
        g = dict(status=int(out.take(np.int32)[0]))
        if g["status"] == 0:
            m = len(c["x"])
            g.update(value=out.take(np.float32, *shape), significant=bool(out.take(np.int32)[0]), r2=out.take(np.float32)[0], parameters=out.take(np.float64, ld.MAX_PARAMETERS),
                     proxy_significant=out.take(np.int32, SLOTS).astype(bool), slope=out.take(np.float64, SLOTS), intercept=out.take(np.float64, SLOTS))
            counts = out.take(np.uint32, 2)
            g.update(fitted=int(counts[0]), kept=int(counts[1]), detrended=out.take(np.float32, m), station_kept=out.take(np.int32, m).astype(bool))
        g["points_status"] = int(out.take(np.int32)[0])
        if g["points_status"] == 0:
            g["points"] = out.take(np.float32, len(c["points"]["x"]))
        o.append(g)
    assert out.done()
    return o


def write_input(path, r, cases) -> None:
    """for the pin's driver (tests/golden/make_multidetrend.py), which reads and writes the program's format"""
    from tests.raster_helpers import write_parts
    write_parts(path, input_parts(r, cases))


def read_output(path, r, cases) -> list:
    return output_of(Path(path).read_bytes(), r, cases)


def run_host(exe, r, directory, cases=None, name=None) -> list:
    """the host program on one raster -> the outcome of every case; the cases run on one block, in order"""
    from tests.raster_helpers import run_host_program
    cases = r["cases"] if cases is None else cases
    return output_of(run_host_program(exe, directory, name or r["name"], input_parts(r, cases)), r, cases)
