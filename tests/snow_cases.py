"""Forcing shared by tests/test_gpu_snow.py, tests/test_snow_host.py and scripts/multirank_snow_worker.py, and the host build of the
kernel's per-cell text (tests/snow_host.cpp) with its runner (no tests here)."""
import numpy as np

from criteria3d_amd import snow


def melt_forcing(shape, dem, flag):
    """a cold snowy day, then a warm hour: every cell holds snow and melts"""
    valid = dem != np.float32(flag)
    def maps_(t, prec, rad):
        f = lambda v: np.where(valid, np.float32(v), np.float32(flag)).astype(np.float32)
        return dict(airT=f(t), prec=f(prec), relHum=f(80.0), windInt=f(2.0), globalRad=f(rad), beamRad=f(rad * 0.7), transmissivity=f(0.6),
                    clearSkyTransmissivity=0.75)
    return [maps_(-3.0, 2.0, 0.0)] * 12 + [maps_(9.0, 1.0, 500.0)] * 4


SHAPES = ((7, 37), (3, 11), (1, 300))          # 259 cells: one block and three lanes; 33: less than a wave; 300: a partial second block
FLAG = -9999.0
# every one of snow.PARAMETER_NAMES away from snow.DEFAULT_PARAMETERS, inside physical ranges
OTHER_PARAMETERS = dict(skinThickness=0.03, soilAlbedo=0.3, snowVegetationHeight=0.5, snowWaterHoldingCapacity=0.08, tempMaxWithSnow=1.5,
                        tempMinWithRain=-1.0, snowSurfaceDampingDepth=0.08)


def small_forcing(shape, seed):
    """(dem, flag, six hours of meteo maps) on a raster of any shape, every cell with values of its own: two cold hours with precipitation
    (snow builds), one hour inside the mixed-precipitation band of the default and of OTHER_PARAMETERS, two warm sunny hours (melt), and one
    hour with the flag (and 0) in relHum, the flag in transmissivity and more than 100 mm of surface water on some cells.  The DEM holds
    the flag in the first and the middle cell and in a few more; the last cell is valid, takes no flag and no free water."""
    rng = np.random.default_rng(seed)
    flag = np.float32(FLAG)
    n = shape[0] * shape[1]
    dem = rng.uniform(50.0, 900.0, shape).astype(np.float32)
    dem[rng.random(shape) < 0.04] = flag
    dem.flat[0] = flag
    dem.flat[n // 2] = flag
    dem.flat[-1] = np.float32(333.0)

    def u(lo, hi, last):
        v = rng.uniform(lo, hi, shape).astype(np.float32)
        v.flat[-1] = np.float32(last)
        return v

    def hour(t, prec, rad, last):
        glob = u(*rad, last[2])
        return dict(airT=u(*t, last[0]), prec=u(*prec, last[1]), relHum=u(45.0, 98.0, 80.0), windInt=u(0.0, 7.0, 2.0), globalRad=glob,
                    beamRad=(glob * np.float32(0.7)).astype(np.float32), transmissivity=u(0.2, 0.74, 0.6), clearSkyTransmissivity=0.75)
    hours = [hour((-9.0, -1.5), (1.0, 5.0), (20.0, 90.0), (-4.0, 3.0, 50.0)), hour((-9.0, -1.5), (1.0, 5.0), (0.0, 0.0), (-4.0, 3.0, 0.0)),
             hour((-0.4, 1.4), (0.5, 4.0), (0.0, 60.0), (0.5, 2.0, 30.0)),
             hour((5.0, 14.0), (0.0, 0.6), (300.0, 800.0), (10.0, 0.2, 600.0)), hour((5.0, 14.0), (0.0, 0.0), (300.0, 800.0), (10.0, 0.0, 600.0)),
             hour((2.5, 9.0), (0.0, 2.0), (50.0, 400.0), (6.0, 1.0, 200.0))]
    h = hours[5]
    pick = rng.random((4,) + shape)
    pick[:, -1, -1] = 1.0
    h["relHum"][pick[0] < 0.15] = flag                       # dew point: no humidity
    h["relHum"][(pick[0] >= 0.15) & (pick[0] < 0.25)] = 0
    h["transmissivity"][pick[1] < 0.2] = flag                # cloud cover default
    water = np.where(pick[2] < 0.15, 150.0, np.where(pick[2] < 0.5, 0.0, rng.uniform(-5.0, 60.0, shape))).astype(np.float32)      # free water above 100 mm
    water.flat[-1] = 0
    h["surfaceWater"] = water
    return dem, float(flag), hours


def restated_run(dem, flag, hours, parameters=None):
    """snow.restate_snow_hour carried along hour by hour from initializeSnowMaps / resetSnowModel under `parameters`: the thirteen maps
    after every hour"""
    fl = np.float32(flag)
    state = snow.restate_reset(np.where(dem == fl, fl, np.float32(0)), flag, parameters)
    out = []
    for met in hours:
        state = snow.restate_snow_hour(state, met, dem, flag, parameters)
        out.append(state)
    return out


# ---- the host build of the per-cell text (tests/snow_host.cpp)

SEEDS = (11, 12, 13, 14)                        # of continuous_forcing, per shape; the device runs the first two


def continuous_forcing(shape, seed):
    """small_forcing's six hours with every map drawn anew from continuous ranges of its own seed, plus a seventh hour whose surface water
    lies between 0 and 120 mm on every cell: (dem, flag, hours).  The share of flag cells and of flags in the inputs is small_forcing's."""
    dem, flag, hours = small_forcing(shape, seed)
    rng = np.random.default_rng(seed + 5000)
    fl = np.float32(flag)
    glob = rng.uniform(0.0, 900.0, shape).astype(np.float32)
    last = dict(airT=rng.uniform(-15.0, 20.0, shape).astype(np.float32), prec=rng.uniform(0.0, 8.0, shape).astype(np.float32),
                relHum=rng.uniform(5.0, 110.0, shape).astype(np.float32), windInt=rng.uniform(0.0, 15.0, shape).astype(np.float32), globalRad=glob,
                beamRad=(glob * rng.uniform(0.0, 1.0, shape).astype(np.float32)).astype(np.float32),
                transmissivity=rng.uniform(0.0, 0.9, shape).astype(np.float32), clearSkyTransmissivity=0.75,
                surfaceWater=rng.uniform(0.0, 120.0, shape).astype(np.float32))
    for name in ("airT", "prec", "globalRad", "beamRad"):
        last[name][rng.random(shape) < 0.04] = fl                    # an invalid point
    return dem, flag, hours + [last]


def run_host(exe, directory, name, dem, flag, state, hours, parameters=None):
    """the host program from `state` (the seven maps by name) over `hours` -> the thirteen maps after every hour, by name"""
    from tests.raster_helpers import Reader, run_host_program
    p = dict(snow.DEFAULT_PARAMETERS)
    p.update(parameters or {})
    n = dem.size
    parts = [np.array([n, len(hours)], np.int32), np.array([flag], np.float32), np.array([p[k] for k in snow.PARAMETER_NAMES], np.float64), dem.astype(np.float32)]
    parts += [np.asarray(state[k], np.float32) for k in snow.STATE]
    for met in hours:
        water = met.get("surfaceWater")
        parts += [np.array([met["clearSkyTransmissivity"]], np.float64), np.array([water is not None], np.int32)]
        parts += [np.asarray(met[k], np.float32) for k in snow.INPUT[:7]]
        if water is not None:
            parts.append(np.asarray(water, np.float32))
    r = Reader(run_host_program(exe, directory, name, parts))
    out = [{k: r.take(np.float32, *dem.shape) for k in snow.STATE + snow.OUTPUT} for _ in hours]
    assert r.done()
    return out


def reset_state(dem, flag, parameters=None):
    """the seven state maps of initializeSnowMaps / resetSnowModel"""
    fl = np.float32(flag)
    m = snow.restate_reset(np.where(dem == fl, fl, np.float32(0)), flag, parameters)
    return {k: m[k] for k in snow.STATE}
