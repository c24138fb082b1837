"""Forcing shared by tests/test_gpu_snow.py and scripts/multirank_snow_worker.py (no tests here)."""
import numpy as np


def melt_forcing(shape, dem, flag):
    """a cold snowy day, then a warm hour: every cell holds snow and melts"""
    valid = dem != np.float32(flag)
    def maps_(t, prec, rad):
        f = lambda v: np.where(valid, np.float32(v), np.float32(flag)).astype(np.float32)
        return dict(airT=f(t), prec=f(prec), relHum=f(80.0), windInt=f(2.0), globalRad=f(rad), beamRad=f(rad * 0.7), transmissivity=f(0.6),
                    clearSkyTransmissivity=0.75)
    return [maps_(-3.0, 2.0, 0.0)] * 12 + [maps_(9.0, 1.0, 500.0)] * 4
