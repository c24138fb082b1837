"""What tests/test_glocal_host.py, tests/test_gpu_glocal.py, tests/golden/make_glocal.py and scripts/multirank_glocal_worker.py share (no
tests here): the pin tests/golden/glocal.npz decoded into its two rasters with their proxy rasters, macro areas, cases and recorded
outcomes; the file format of the host build of the kernels' text (tests/glocal_host.cpp), which the pin's driver reads and writes too; the
calls of a case through the binding and through the restatement; and, away from the pin, `synthetic`: area lists of 65 and 130 stations,
five areas, 31 first guesses, a cell under five areas (OFF_PIN); the edges of the lists and of the areas (OFF_PIN_EDGES: stations of an
area without a point this hour, lists of 2 to 1024 stations, one, eight, nine and ten areas, an area with no point at all, no retrend),
each row with the property the host build's outcome must show; and `failing_area` and `failing_single_station`, in which an interpolate()
gives NODATA.

A raster carries SLOTS proxy slots as tests/localproxies_cases.py's do, and its macro areas: per area dict(cells, weights, stations).  A
case adds the index of every point to a case of localproxies_cases."""
import json
from pathlib import Path

import numpy as np

from criteria3d_amd import glocal as gl, localdetrend as ld, meteo
from tests import localdetrend_cases as lc, localproxies_cases as pc

ROOT = Path(__file__).resolve().parent.parent
PIN = ROOT / "tests" / "golden" / "glocal.npz"
RASTERS = ("relief", "tiny")
SLOTS = pc.SLOTS
PORT = 29805                                    # the two-rank test's (clear of tests/ranks.py's table and of the other blocks' ports)
# the rule of tests/raster_helpers.py same for every recorded quantity
QUANTITIES = dict(value="bits", significant="value", r2="nan", parameters="nan", proxy_significant="value", slope="nan", intercept="nan", fitted="value",
                  kept="value", detrended="bits", station_kept="value")
AREA_QUANTITIES = {k: v for k, v in QUANTITIES.items() if k != "value"}

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
        r["areas"] = unflatten(p[f"{name}_cell_offset"], p[f"{name}_cell"], p[f"{name}_weight"], p[f"{name}_station_offset"], p[f"{name}_station_index"])
        na = len(r["areas"])
        for k, c in enumerate(json.loads(str(p[f"{name}_cases"]))):
            g = lambda key: p[f"{name}_c{k}_{key}"]
            n_par = len(c["fit"]["min"])
            par = np.full((na, ld.MAX_PARAMETERS), ld.NODATA, np.float64)
            par[:, :n_par] = g("par")
            c.update(point_index=g("index"), x=g("x"), y=g("y"), proxy_values=g("pv"), value=g("v"), area=np.float32(c["area"]),
                     want=dict(value=g("map"), significant=g("sig").astype(bool), r2=g("r2"), parameters=par, proxy_significant=g("psig").astype(bool), slope=g("slope"),
                               intercept=g("icpt"), fitted=g("fitted").astype(np.uint32), kept=g("kept").astype(np.uint32), detrended=g("det"),
                               station_kept=g("skept").astype(bool)))
            r["cases"].append(c)
        out[name] = r
    return out


def unflatten(cell_offset, cell, weight, station_offset, station_index) -> list:
    return [dict(cells=np.asarray(cell[cell_offset[a]:cell_offset[a + 1]], np.float32), weights=np.asarray(weight[cell_offset[a]:cell_offset[a + 1]], np.float32),
                 stations=np.asarray(station_index[station_offset[a]:station_offset[a + 1]], np.int32)) for a in range(len(cell_offset) - 1)]


def restated(r, c, mine=None, arms=None) -> dict:
    return gl.restate_interpolate(r["dem"], r["xll"], r["yll"], r["cell_size"], maps_of(r), r["areas"], c["var"], c["method"], c["point_index"], c["x"], c["y"], c["value"],
                                  c["proxy_values"], c["area"], c["fit"], proxies_of(c), c["others"], dict(useDetrending=c["useDetrending"]), float(r["flag"]), mine, arms)


def initialize(sf, r) -> None:
    pc.initialize(sf, r)
    gl.set_areas(sf, r["areas"])


def interpolate(sf, c, download=True):
    return gl.interpolate(sf, c["var"], c["method"], c["point_index"], c["x"], c["y"], c["value"], c["proxy_values"], c["area"], c["fit"], proxies_of(c), c["others"],
                          dict(useDetrending=c["useDetrending"]), download)


def outcome(sf, value) -> dict:
    """the map with what the getter returns of the last call, by the names of QUANTITIES"""
    return dict(value=value, **gl.get_area_fit(sf))


# ---- away from the pin

def strip_areas(shape, n_areas: int, n_stations: int, lists, rng, everywhere=()) -> list:
    """n_areas areas over a raster: area a covers a band of columns that overlaps its neighbours', with weights that fall off from the
    band's middle and do not add up to 1; lists[a]: how many stations it names (the first ones of a seeded shuffle); everywhere: areas
    that cover every cell"""
    rows, cols = shape
    out = []
    for a in range(n_areas):
        lo, hi = (0, cols) if a in everywhere else (max(0, int((a - 0.6) * cols / n_areas)), min(cols, int((a + 1.6) * cols / n_areas)))
        cells, weights = [], []
        for r in range(rows):
            for c in range(lo, hi):
                cells.append(np.float32(r * cols + c))
                weights.append(np.float32(round(0.25 + 0.6 * (1.0 - abs((c - (lo + hi - 1) / 2.0) / max(1.0, (hi - lo) / 2.0))), 3)))
        stations = rng.permutation(n_stations)[:lists[a]].astype(np.int32)
        out.append(dict(cells=np.array(cells, np.float32), weights=np.array(weights, np.float32), stations=stations))
    return out


def without_points(c, keep) -> dict:
    """the case with the call's point table cut to `keep` (a mask over the points): the areas stay as they are, so the list of an area
    that names a point cut here has an entry without a point this hour"""
    keep = np.asarray(keep, bool)
    return dict(c, point_index=c["point_index"][keep], x=c["x"][keep], y=c["y"][keep], value=c["value"][keep], proxy_values=c["proxy_values"][:, keep])


def missing_points(r, c, rule) -> np.ndarray:
    """the mask `without_points` takes, by a rule: ("every", k): the call's points 0, k, 2 k, ... have gone; ("entries", a, lo, hi): the
    stations that area a's list names at positions lo to hi - 1 have no point"""
    keep = np.ones(len(c["point_index"]), bool)
    if rule[0] == "every":
        keep[::rule[1]] = False
    elif rule[0] == "entries":
        _, a, lo, hi = rule
        keep[np.isin(c["point_index"], r["areas"][a]["stations"][lo:hi])] = False
    else:
        raise ValueError(f"no rule {rule!r}")
    return keep


def synthetic(n_stations: int, lists, method: int, n_others: int, function: int = ld.PIECEWISE_TWO, guesses: int | None = 2, seed: int = 3, everywhere=(),
              position=None, use_detrending: int = 1, var: int = meteo.AIR_TEMPERATURE, empty_areas=(), missing=None) -> tuple:
    """(raster, case) away from the pin: localproxies_cases.synthetic's 3 x 11 raster, stations and proxies with len(lists) strip areas
    and shuffled point indices; position: the first-guess positions (None: localdetrend_cases.synthetic's); empty_areas: (position,
    station ids that are in no call) of areas without cells put in among the strip areas; missing: a rule of `missing_points`, applied
    once the areas stand"""
    r, c = pc.synthetic(n_stations, 5, method, n_others, seed, function, guesses)
    if position is not None:
        c["fit"] = lc.synthetic(n_stations, 5, method, function, guesses, position=position)[1]["fit"]
    rng = np.random.default_rng(seed * 1000 + n_stations)
    r["areas"] = strip_areas(r["dem"].shape, len(lists), n_stations, lists, rng, everywhere)
    c["point_index"] = (np.arange(n_stations, dtype=np.int32) * 3 + 7)[rng.permutation(n_stations)]
    for a in r["areas"]:
        a["stations"] = c["point_index"][a["stations"]].astype(np.int32)
    c["fit"] = dict(c["fit"], minPointsLocalDetrending=0)
    c["useDetrending"], c["var"] = use_detrending, var
    for at, ids in empty_areas:
        assert not np.isin(ids, c["point_index"]).any()
        r["areas"].insert(at, dict(cells=np.zeros(0, np.float32), weights=np.zeros(0, np.float32), stations=np.array(ids, np.int32)))
    if missing is not None:
        c = without_points(c, missing_points(r, c, missing))
    return r, c


def _off_pin() -> tuple:
    I, S, M = meteo.IDW, meteo.SHEPARD, meteo.SHEPARD_MODIFIED
    return (
        # an area list of 65 and one of 130 stations: one and two wave widths crossed; five areas: the second block has one wave idle
        ("lists65-130", dict(n_stations=140, lists=(65, 130, 30, 64, 12), method=I, n_others=2)),
        ("lists-modified", dict(n_stations=140, lists=(65, 130, 30, 64, 12), method=M, n_others=3)),
        # 31 first guesses of the three-piece functions: parameters 0 and 2 both walked up from their minima
        ("guesses31-three", dict(n_stations=40, lists=(40, 25, 33), method=S, n_others=1, function=ld.PIECEWISE_THREE, guesses=31, position=[0, 0, 1, 1, 1])),
        ("guesses31-free", dict(n_stations=40, lists=(28, 40), method=I, n_others=0, function=ld.PIECEWISE_THREE_FREE, guesses=31, position=[0, 0, 1, 1, 1, 1])),
        # every cell under five areas
        ("five-deep", dict(n_stations=60, lists=(20, 30, 40, 50, 60), method=I, n_others=2, everywhere=(0, 1, 2, 3, 4))),
    )


OFF_PIN = _off_pin()


# ---- the edges of the lists and of the areas: what the host build's outcome g of a row must show, so that a row cannot stop reaching its
# edge unnoticed.  The numbers are the host build's (held to the restatement by tests/test_glocal_host.py), never a device's.
# must(r, c, g, again): again(**changes): the host build's outcome of the row with those arguments of `synthetic` changed

def lengths(r) -> list:
    return [len(a["stations"]) for a in r["areas"]]


def entries(r, a: int) -> slice:
    """area a's entries in the per-entry quantities (detrended, station_kept)"""
    first = sum(lengths(r)[:a])
    return slice(first, first + len(r["areas"][a]["stations"]))


def _holes(r, c, g, again):
    assert g["status"] == 0 and (g["fitted"] < np.array(lengths(r))).all() and (g["fitted"] > 0).all(), g["fitted"]


def _holes_third(r, c, g, again):
    _holes(r, c, g, again)
    assert (g["kept"] < g["fitted"]).any() and g["proxy_significant"][:, 1:].any()
    assert g["fitted"].tolist() == [43, 85, 24, 44, 8]
    if c["method"] == meteo.IDW:
        assert g["kept"].tolist() == [39, 79, 23, 40, 8]


def _holes_run64(r, c, g, again):
    _holes(r, c, g, again)
    assert not np.isin(r["areas"][1]["stations"][:64], c["point_index"]).any()       # the ballot of area 1's first chunk is 0
    assert np.isin(r["areas"][1]["stations"][64:], c["point_index"]).all()
    assert g["fitted"].tolist() == [36, 66, 20, 29, 7]


def _holes_tail(r, c, g, again):
    _holes(r, c, g, again)
    assert len(r["areas"][1]["stations"]) == 130 and 1 <= g["fitted"][1] <= 2
    kept = g["station_kept"][entries(r, 1)]
    assert kept.any() and not kept[:128].any()


def _full(r, c, g, again):
    assert g["status"] == 0 and g["fitted"].tolist() == lengths(r)


def _wave_edges(r, c, g, again):
    _full(r, c, g, again)
    assert lengths(r) == [63, 127, 128, 129, 64]


def _cap(r, c, g, again):
    _full(r, c, g, again)
    assert lengths(r) == [meteo.MAX_STATIONS, 1023, 257, 256, 255] and g["kept"].tolist() == [964, 963, 245, 246, 242] and g["significant"].all()


def _small(r, c, g, again):
    _full(r, c, g, again)
    assert lengths(r) == [2, 4, 5, 6, 30] and g["significant"].tolist()[:2] == [False, False] and g["kept"].tolist() == [2, 4, 5, 6, 28]


def _neighbourhood(r, c, g, again):
    _full(r, c, g, again)
    assert g["kept"][0] == 5 and g["kept"][2] == 11 and g["kept"][1] in (8, 10), g["kept"]


def _records(n: int):
    def must(r, c, g, again):
        _full(r, c, g, again)
        assert len(r["areas"]) == n and all(len(g[q]) == n for q in ("fitted", "kept", "significant", "r2", "parameters", "slope"))
    return must


def _empty(r, c, g, again):
    assert g["status"] == 0 and len(r["areas"]) == 10 and len(r["areas"][4]["cells"]) == 0 and len(r["areas"][4]["stations"]) == 3
    assert g["fitted"][4] == 0 and g["kept"][4] == 0 and not g["significant"][4] and not g["proxy_significant"][4].any()
    assert (g["parameters"][4] == ld.NODATA).all() and g["r2"][4] == np.float32(ld.NODATA) and not g["station_kept"][entries(r, 4)].any()
    others = [a for a in range(10) if a != 4]
    assert g["fitted"][others].tolist() == [lengths(r)[a] for a in others]


def _no_retrend(r, c, g, again):
    assert g["status"] == 0 and c["useDetrending"] == 0
    with_it = again(use_detrending=1)
    assert with_it["status"] == 0 and (bits_of(g["value"]) != bits_of(with_it["value"])).any()
    assert g["significant"].any() or g["proxy_significant"].any()


def _dew_holes(r, c, g, again):
    _holes(r, c, g, again)
    assert c["var"] == meteo.AIR_DEW_TEMPERATURE and c["fit"]["function"] == ld.PIECEWISE_THREE_FREE and len(c["fit"]["first_guess"]) == 31


def bits_of(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


EMPTY_IDS = (8, 9, 11)                          # the point indices are 7, 10, 13, ...: in no call


def _off_pin_edges() -> tuple:
    """(label, the arguments of `synthetic` by name, what the host build's outcome must show)"""
    I, S, M = meteo.IDW, meteo.SHEPARD, meteo.SHEPARD_MODIFIED
    name = meteo.METHODS
    five, cap = (65, 130, 30, 64, 12), (meteo.MAX_STATIONS, 1023, 257, 256, 255)
    nine = (20, 30, 40, 50, 60, 70, 80, 10, 15)
    out = [
        # entries without a point this hour: a ballot with gaps in every chunk, the count carried across chunks off the chunk's base
        ("holes-third", dict(n_stations=140, lists=five, method=I, n_others=2, missing=("every", 3)), _holes_third),
        ("holes-third-modified", dict(n_stations=140, lists=five, method=M, n_others=3, missing=("every", 3)), _holes_third),
        # a chunk whose ballot is 0: the first of the list of 130
        ("holes-run64-idw", dict(n_stations=140, lists=five, method=I, n_others=2, missing=("entries", 1, 0, 64)), _holes_run64),
        ("holes-run64-shepard", dict(n_stations=140, lists=five, method=S, n_others=2, missing=("entries", 1, 0, 64)), _holes_run64),
        # two chunks whose ballot is 0, then a third of two entries (the twelve stations left keep every other area legal)
        ("holes-tail", dict(n_stations=140, lists=five, method=I, n_others=2, missing=("entries", 1, 0, 128)), _holes_tail),
        # list lengths at the wave's edges, and at METEO_MAX_STATIONS, which the LDS arrays of k_glocal_areas are sized for
        ("lists-wave-edges", dict(n_stations=140, lists=(63, 127, 128, 129, 64), method=I, n_others=2), _wave_edges),
        ("lists-cap", dict(n_stations=meteo.MAX_STATIONS, lists=cap, method=I, n_others=2), _cap),
        ("lists-cap-holes", dict(n_stations=meteo.MAX_STATIONS, lists=cap, method=I, n_others=2, missing=("every", 5)), _holes),
    ]
    # areas below the five stations of proxyValidity and below the Shepard neighbourhood's minimum
    out += [(f"small-lists-{name[m]}", dict(n_stations=30, lists=(2, 4, 5, 6, 30), method=m, n_others=1), _small) for m in (I, S, M)]
    out += [(f"neighbourhood-edges-{name[m]}", dict(n_stations=30, lists=(5, 10, 11, 30), method=m, n_others=1), _neighbourhood) for m in (S, M)]
    out += [
        # one wave of one block; two full blocks; a third block of one wave
        ("one-area", dict(n_stations=70, lists=(70,), method=M, n_others=2, everywhere=(0,)), _records(1)),
        ("eight-areas", dict(n_stations=80, lists=nine[:8], method=I, n_others=1), _records(8)),
        ("nine-areas", dict(n_stations=80, lists=nine, method=I, n_others=1), _records(9)),
        # the n == 0 path of gl_area beside three busy waves of its block
        ("empty-area", dict(n_stations=80, lists=nine, method=I, n_others=1, empty_areas=((4, EMPTY_IDS),)), _empty),
    ]
    out += [(f"no-retrend-{name[m]}", dict(dict(OFF_PIN)["five-deep"], method=m, use_detrending=0), _no_retrend) for m in (I, S)]
    out.append(("dew-free-holes", dict(dict(OFF_PIN)["guesses31-free"], var=meteo.AIR_DEW_TEMPERATURE, missing=("every", 4)), _dew_holes))
    return tuple(out)


OFF_PIN_EDGES = _off_pin_edges()
EDGE_LABELS = tuple(row[0] for row in OFF_PIN_EDGES)


def off_pin(label: str) -> tuple:
    r, c = synthetic(**{row[0]: row[1] for row in OFF_PIN + OFF_PIN_EDGES}[label])
    r["name"], c["label"] = label, label
    return r, c


# the sparsity of `holes-tail` on the areas of `lists-cap`: of the list of 1024 only the last chunk has points
CAP_TAIL = ("entries", 0, 0, meteo.MAX_STATIONS - 64)


def failing_area() -> tuple:
    """(raster, case) in which an interpolate() of the cell loop gives NODATA: the six stations of area 1 sit on the centre of cell
    (1, 9), which area 1 alone covers, so every distance is 0 there and inverseDistanceWeighted has no weight to divide by.  (An area
    whose rebuilt subset detrendingOtherProxies erases whole cannot be built: a proxy is significant only with five values in the fit,
    and the stations that carry them survive step 2 - DESIGN.md 26.)"""
    r, c = synthetic(n_stations=24, lists=(24, 6), method=meteo.IDW, n_others=1)
    # area 1's six stations sit on the centre of cell (1, 9), which only area 1 covers: every distance is 0 there
    cx, cy = meteo.cell_centres(r["dem"].shape, r["xll"], r["yll"], r["cell_size"])
    index = list(c["point_index"])
    for s in r["areas"][1]["stations"]:
        k = index.index(int(s))
        c["x"][k], c["y"][k] = cx[1, 9], cy[1, 9]
    cols = r["dem"].shape[1]
    r["areas"][1]["cells"], r["areas"][1]["weights"] = np.array([1 * cols + 9], np.float32), np.array([0.7], np.float32)
    keep = r["areas"][0]["cells"] != np.float32(1 * cols + 9)
    r["areas"][0]["cells"], r["areas"][0]["weights"] = r["areas"][0]["cells"][keep], r["areas"][0]["weights"][keep]
    r["name"], c["label"] = "failed", "failed"
    return r, c


def failing_single_station(method: int) -> tuple:
    """(raster, case) in which both Shepard methods give NODATA: area 0 names one station and covers the raster's first columns alone"""
    r, c = synthetic(n_stations=30, lists=(1, 30), method=method, n_others=1)
    alone = np.setdiff1d(r["areas"][0]["cells"], r["areas"][1]["cells"])
    assert method != meteo.IDW and (r["dem"].ravel()[alone.astype(int)] != r["flag"]).any()
    r["name"] = c["label"] = f"failed-single-{meteo.METHODS[method]}"
    return r, c


# ---- the file format of tests/glocal_host.cpp (its header comment)

def input_parts(r, cases, options=None) -> list:
    """r["areas"] None: the file of a program that never sets the areas"""
    if r["areas"] is None:
        e = np.zeros(0, np.uint32)
        f = dict(cell_offset=e, cell=e.astype(np.float32), weight=e.astype(np.float32), station_offset=e, station_index=e.astype(np.int32))
    else:
        f = gl.flat_areas(r["areas"])
    parts = [np.array([r["dem"].shape[0], r["dem"].shape[1], len(cases)], np.int32), np.array([r["flag"]], np.float32),
             np.array([r["xll"], r["yll"], r["cell_size"]], np.float64), r["dem"].astype(np.float32), np.asarray(r["maps"], np.float32),
             np.array([-1 if r["areas"] is None else len(r["areas"]), len(f["cell"]), len(f["station_index"])], np.int32), f["cell_offset"], f["cell"], f["weight"], f["station_offset"], f["station_index"]]
    for c in cases:
        o = dict(useMultipleDetrending=1, useLocalDetrending=0, nProxies=SLOTS)
        o.update(c.get("options", {}))
        o.update(options or {})
        parts += [lc.case_head(c), np.array([o["useMultipleDetrending"], o["useLocalDetrending"], o["nProxies"]], np.int32), np.array(c["active"], np.int32),
                  np.array([c["fit"]["stdDevThreshold"], c["area"]], np.float32), np.array([o["stdDevThreshold"] for o in c["others"]], np.float32),
                  np.array([list(o["min"]) + list(o["max"]) for o in c["others"]], np.float64), lc.fit_table(c["fit"]), np.asarray(c["point_index"], np.int32),
                  np.asarray(c["x"], np.float64), np.asarray(c["y"], np.float64), np.asarray(c["proxy_values"], np.float32), np.asarray(c["value"], np.float32)]
    return parts


def output_of(raw: bytes, r, cases) -> list:
    """per case dict(status, and where status < 2 the quantities); None in the place of the list: the areas are refused"""
    from tests.raster_helpers import Reader
    shape, out, o = r["dem"].shape, Reader(raw), []
    if int(out.take(np.int32)[0]) == 0:
        assert out.done()
        return None
    na, nl = len(r["areas"] or ()), sum(len(a["stations"]) for a in r["areas"] or ())
    for _ in cases:
        status = int(out.take(np.int32)[0])
        if status == 2:
            o.append(dict(status=2))
            continue
        o.append(dict(status=status, value=out.take(np.float32, *shape), significant=out.take(np.int32, na).astype(bool), r2=out.take(np.float32, na),
                      parameters=out.take(np.float64, na, ld.MAX_PARAMETERS), proxy_significant=out.take(np.int32, na, SLOTS).astype(bool),
                      slope=out.take(np.float64, na, SLOTS), intercept=out.take(np.float64, na, SLOTS), fitted=out.take(np.uint32, na), kept=out.take(np.uint32, na),
                      detrended=out.take(np.float32, nl), station_kept=out.take(np.int32, nl).astype(bool)))
    assert out.done()
    return o


def write_input(path, r, cases) -> None:
    """for the pin's driver (tests/golden/make_glocal.py), which reads and writes the program's format"""
    from tests.raster_helpers import write_parts
    write_parts(path, input_parts(r, cases))


def read_output(path, r, cases) -> list:
    return output_of(Path(path).read_bytes(), r, cases)


def run_host(exe, r, directory, cases=None, name=None) -> list:
    """the host program on one raster -> the outcome of every case"""
    from tests.raster_helpers import run_host_program
    cases = r["cases"] if cases is None else cases
    return output_of(run_host_program(exe, directory, name or r["name"], input_parts(r, cases)), r, cases)
