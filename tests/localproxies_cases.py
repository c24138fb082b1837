"""What tests/test_localproxies_host.py, tests/test_gpu_localproxies.py, tests/golden/make_localproxies.py and
scripts/multirank_localproxies_worker.py share (no tests here): the pin tests/golden/localproxies.npz decoded into its two rasters with
their proxy rasters, cases and recorded outcomes; the file format of the host build of the per-cell text (tests/localproxies_host.cpp),
which the pin's driver reads and writes too; the calls of a case through the binding and through the restatement; and, away from the pin,
`synthetic` with the table OFF_PIN of its arguments: one to seven other proxies all significant (5, 14, 27, 44, 65, 90, 119 entries of the
normal matrix and the gradient) on lists of 14 to 31 and of 70, the three-piece functions and an inactive height under them, and mixed
significance on lists of 70 and of 122 to 131.

A raster carries SLOTS proxy slots: slot 0 is the height (no raster of its own: the DEM), slots 1 .. 7 hold the synthetic rasters.  A
case says which slots are active, the stations' value of every slot, and range and threshold of every slot that is not the height."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import localdetrend as ld, localproxies as lp, meteo
from tests import localdetrend_cases as lc

ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "localproxies.npz"
RASTERS = ("relief", "tiny")
SLOTS = meteo.MAX_PROXIES
PORT = 29803                                    # the two-rank test's (clear of tests/ranks.py's table and of the other blocks' ports)
# the rule of tests/raster_helpers.py same for every recorded quantity: a NaN equal to any NaN in R2 and in the doubles of the fits
QUANTITIES = dict(value="bits", count="value", interpolated="value", radius="bits", significant="value", r2="nan", parameters="nan", proxy_significant="value",
                  slope="nan", intercept="nan")


def proxies_of(c) -> list:
    return [dict(active=int(a), isHeight=int(k == 0)) for k, a in enumerate(c["active"])]


def maps_of(r) -> list:
    """the rasters of meteo.initialize: None in the height's slot"""
    return [None] + [r["maps"][k] for k in range(1, SLOTS)]


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
            par = np.full(r["dem"].shape + (ld.MAX_PARAMETERS,), ld.NODATA, np.float64)
            par[..., :n_par] = g("par")
            c.update(x=g("x"), y=g("y"), proxy_values=g("pv"), value=g("v"), area=np.float32(c["area"]),
                     want=dict(value=g("map"), count=g("count").astype(np.uint32), interpolated=g("interp").astype(np.uint32), radius=g("radius"),
                               significant=g("sig").astype(bool), r2=g("r2"), parameters=par, proxy_significant=g("psig").astype(bool), slope=g("slope"),
                               intercept=g("icpt")))
            r["cases"].append(c)
        out[name] = r
    return out


def case_name(c) -> str:
    active = "".join(str(int(a)) for a in c["active"])
    return f"{c['label']}-{meteo.VARIABLES[c['var']]}-{meteo.METHODS[c['method']]}-{ld.FUNCTIONS[c['fit']['function']]}-min{c['fit']['minPointsLocalDetrending']}-{active}"


def restated(r, c, mine=None, arms=None) -> dict:
    return lp.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], maps_of(r), c["var"], c["method"], c["x"], c["y"], c["value"], c["proxy_values"],
                                  c["area"], c["fit"], proxies_of(c), c["others"], dict(useDetrending=c["useDetrending"]), float(r["flag"]), mine, arms)


def initialize(sf, r) -> None:
    meteo.initialize(sf, r["dem"], r["xll"], r["yll"], r["cell_size"], maps_of(r), float(r["flag"]))


def interpolate(sf, c, download=True):
    return lp.interpolate(sf, c["var"], c["method"], c["x"], c["y"], c["value"], c["proxy_values"], c["area"], c["fit"], proxies_of(c), c["others"],
                          dict(useDetrending=c["useDetrending"]), download)


def outcome(sf, value) -> dict:
    """the map with what the getters return of the last call, by the names of QUANTITIES"""
    return dict(value=value, interpolated=lp.get_interpolated(sf), **ld.get_selection(sf), **ld.get_fit(sf), **lp.get_proxy_fit(sf))


def default_others(threshold=ld.NODATA) -> list:
    """the reference's default range of a proxy without one ({-1, -40, 1, 50}, interpolationSettings.cpp:251) in every slot beside the height's"""
    return lp.make_others([None] + [dict(range=[-1.0, -40.0, 1.0, 50.0], stdDevThreshold=threshold)] * (SLOTS - 1))


def synthetic_rasters(shape, rng) -> np.ndarray:
    """SLOTS rasters on `shape` (slot 0 unused): a plane, a patchy 0 / fraction map with flag holes, a bounded index, and four more of the
    three kinds"""
    rows, cols = shape
    r, c = np.mgrid[0:rows, 0:cols]
    maps = np.zeros((SLOTS,) + shape, np.float32)
    maps[1] = np.round(2.0 + 0.45 * c + 0.3 * r, 2)                                           # sea distance [km]: a plane
    urban = np.where(rng.uniform(size=shape) < 0.45, np.round(rng.uniform(0.05, 1.0, shape), 2), 0.0)
    maps[2] = urban
    maps[3] = np.round(np.sin(0.7 * c) * np.cos(0.9 * r), 3)                                  # a bounded index
    maps[4] = np.round(1.0 / (1.0 + np.exp(-(c - cols / 2.0) / 3.0)), 3)                       # water index
    maps[5] = np.round(30.0 - 0.6 * c + 0.8 * r, 2)                                           # another plane
    maps[6] = np.where(rng.uniform(size=shape) < 0.3, np.round(rng.uniform(0.1, 1.0, shape), 2), 0.0)
    maps[7] = np.round(np.cos(0.4 * c + 0.5 * r), 3)
    return maps.astype(np.float32)


def synthetic(n_stations: int, min_points_local: int, method: int, n_others: int, seed: int = 11, function: int = ld.PIECEWISE_TWO, guesses: int | None = 2,
              height_seed: int = 7, height_active: bool = True, thresholds=None, spoil=None) -> tuple:
    """(raster, case) away from the pin: the 3 x 11 raster of localdetrend_cases.synthetic(.., function, guesses, height_seed) with proxy
    rasters, `n_stations` stations and `n_others` other proxies active beside the height; the stations' proxy values have trends in them,
    some are 0 and a few NODATA.  thresholds: {slot: stdDevThreshold}; spoil: {slot: "nodata" (four stations keep a value: too few for
    proxyValidity) or "constant" (one value everywhere: with a threshold, no deviation)}"""
    r, c = lc.synthetic(n_stations, min_points_local, method, function, guesses, height_seed)
    rng = np.random.default_rng(seed + n_stations + n_others)
    r["maps"] = synthetic_rasters(r["dem"].shape, rng)
    r["maps"][2][0, 3] = r["flag"]
    pv = np.zeros((SLOTS, n_stations), np.float32)
    pv[0] = c.pop("height")
    t = c["value"].astype(np.float64)
    for k in range(1, SLOTS):
        if k in (2, 6):
            v = np.where(rng.uniform(size=n_stations) < 0.5, np.round(rng.uniform(0.05, 1.0, n_stations), 2), 0.0)
        else:
            v = np.round(rng.uniform(0.0, 40.0, n_stations), 2)
        pv[k] = v
        t = t + (0.03 * k) * v * (1 if k % 2 else -1)
    pv[1][5::17] = np.float32(ld.NODATA)
    pv[3][2::23] = np.float32(ld.NODATA)
    for k, how in (spoil or {}).items():
        if how == "nodata":
            pv[k][4:] = np.float32(ld.NODATA)
        else:
            pv[k][:] = np.float32(3.25)
    c["value"] = np.round(t, 1).astype(np.float32)
    c["proxy_values"] = pv
    c["active"] = [int(height_active)] + [1] * n_others + [0] * (SLOTS - 1 - n_others)
    c["others"] = default_others()
    for k, threshold in (thresholds or {}).items():
        c["others"][k] = dict(c["others"][k], stdDevThreshold=float(threshold))
    return r, c


def _off_pin() -> tuple:
    """(label, the arguments of `synthetic` by name).  k significant other proxies make NP (NP + 1) / 2 + NP entries of the normal matrix
    and the gradient with NP = 2 k: 5, 14, 27, 44, 65, 90, 119 - a lane of the wave owns the entries lane and lane + 64, so k = 5 is the one
    shape in which lane 0 alone owns a second entry"""
    I, M = meteo.IDW, meteo.SHEPARD_MODIFIED
    out = []
    # every k, all significant in every cell: a list within a wave, and a list of 70 whose interpolated list ends around 64
    for n, mpl in ((40, 12), (70, 60)):
        for k in range(1, lp.MAX_OTHERS + 1):
            out.append((f"all{n}-k{k}", dict(n_stations=n, min_points_local=mpl, method=I, n_others=k)))
    # the three-piece functions under the proxies, more than two busy fit lanes
    out.append(("three70-k5", dict(n_stations=70, min_points_local=60, method=M, n_others=5, function=ld.PIECEWISE_THREE, guesses=3)))
    out.append(("free70-k5", dict(n_stations=70, min_points_local=60, method=I, n_others=5, function=ld.PIECEWISE_THREE_FREE, guesses=4)))
    out.append(("three70-k6", dict(n_stations=70, min_points_local=60, method=I, n_others=6, function=ld.PIECEWISE_THREE, guesses=4)))
    out.append(("free70-k6", dict(n_stations=70, min_points_local=60, method=M, n_others=6, function=ld.PIECEWISE_THREE_FREE, guesses=3)))
    out.append(("noheight70-k3", dict(n_stations=70, min_points_local=60, method=M, n_others=3, height_active=False)))
    out.append(("modified40-k5", dict(n_stations=40, min_points_local=12, method=M, n_others=5)))
    # mixed significance on long lists: thresholds, a slot with four values, a constant slot - the significant slots have gaps
    out.append(("mixed70", dict(n_stations=70, min_points_local=60, method=M, n_others=7, thresholds={2: 1.0, 5: 100.0}, spoil={4: "nodata"})))
    out.append(("mixed150", dict(n_stations=150, min_points_local=60, method=I, n_others=6, thresholds={1: 11.65, 2: 0.5, 3: 11.1, 6: 0.335}, spoil={2: "constant"})))
    out.append(("none70", dict(n_stations=70, min_points_local=60, method=I, n_others=4, thresholds={1: 100.0, 2: 100.0, 3: 100.0, 4: 100.0})))
    return tuple(out)


OFF_PIN = _off_pin()
# the restatement takes more than 5 s on these: held host build against device only (the same functions at k = 6 are restated)
HOST_ONLY = ("three70-k5", "free70-k5")


def off_pin(label: str) -> tuple:
    r, c = synthetic(**dict(OFF_PIN)[label])
    r["name"], c["label"] = label, label
    return r, c


# ---- the file format of tests/localproxies_host.cpp (its header comment)

def input_parts(r, cases) -> list:
    parts = [np.array([r["dem"].shape[0], r["dem"].shape[1], len(cases)], np.int32), np.array([r["flag"]], np.float32),
             np.array([r["xll"], r["yll"], r["cell_size"]], np.float64), r["dem"].astype(np.float32), np.asarray(r["maps"], np.float32)]
    for c in cases:
        parts += [lc.case_head(c), np.array(c["active"], np.int32), np.array([c["fit"]["stdDevThreshold"], c["area"]], np.float32),
                  np.array([o["stdDevThreshold"] for o in c["others"]], np.float32), np.array([list(o["min"]) + list(o["max"]) for o in c["others"]], np.float64),
                  lc.fit_table(c["fit"]), np.asarray(c["x"], np.float64), np.asarray(c["y"], np.float64), np.asarray(c["proxy_values"], np.float32),
                  np.asarray(c["value"], np.float32)]
    return parts


def output_of(raw: bytes, r, cases) -> list:
    from tests.raster_helpers import Reader
    shape, out, o = r["dem"].shape, Reader(raw), []
    for _ in cases:
        o.append(dict(value=out.take(np.float32, *shape), count=out.take(np.uint32, *shape), interpolated=out.take(np.uint32, *shape), radius=out.take(np.float32, *shape),
                      significant=out.take(np.int32, *shape).astype(bool), r2=out.take(np.float32, *shape), parameters=out.take(np.float64, *shape, ld.MAX_PARAMETERS),
                      proxy_significant=out.take(np.int32, *shape, SLOTS).astype(bool), slope=out.take(np.float64, *shape, SLOTS),
                      intercept=out.take(np.float64, *shape, SLOTS)))
    assert out.done()
    return o


def write_input(path, r, cases) -> None:
    """for the pin's driver (tests/golden/make_localproxies.py), which reads and writes the program's format"""
    from tests.raster_helpers import write_parts
    write_parts(path, input_parts(r, cases))


def read_output(path, r, cases) -> list:
    return output_of(Path(path).read_bytes(), r, cases)


def run_host(exe, r, directory, cases=None) -> list:
    """the host program on one raster -> the outcome of every case"""
    from tests.raster_helpers import run_host_program
    cases = r["cases"] if cases is None else cases
    return output_of(run_host_program(exe, directory, r["name"], input_parts(r, cases)), r, cases)
