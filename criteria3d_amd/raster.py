"""What the Python bindings of the raster blocks (snow.py, crop.py, root.py, meteo.py, sinks.py) share: maps checked against the raster's
shape, names of state maps, and the folder of ESRI float grids a block's state is saved to."""
from __future__ import annotations

from functools import partial
from pathlib import Path

import numpy as np

from . import esri


def _map(a, shape=None, what: str = "", dtype=np.float32):
    """`a` as a contiguous array of `dtype`; ValueError when it is not of the `what` raster's shape"""
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"map of shape {a.shape}, the {what} raster is {tuple(shape)}")
    return a


f32 = partial(_map, dtype=np.float32)          # a float map
i32 = partial(_map, dtype=np.int32)            # an index map


def index(which, names) -> int:
    return names.index(which) if isinstance(which, str) else int(which)


def save_state(directory, folder: str, files: dict, get, header: dict) -> Path:
    """<directory>/<folder>/<stem>.flt/.hdr for every (name, stem) of `files`, the map from get(name)"""
    d = Path(directory) / folder
    d.mkdir(parents=True, exist_ok=True)
    for name, stem in files.items():
        esri.write_grid(d / stem, get(name), header)
    return d


def load_state(directory, folder: str, files: dict, put) -> None:
    """the grids save_state wrote, each handed to put(name, grid)"""
    d = Path(directory) / folder
    for name, stem in files.items():
        grid, _ = esri.read_grid(d / stem)
        put(name, grid)
