#!/usr/bin/env python3
"""Generate tests/golden/ravone_geotechnics.json: the slope-stability data of SOIL/soil_ER_2021.db of the Ravone project (BASELINE
config 5) as data.  Build container only (the reference's database is read read-only):

    python tests/golden/make_ravone_geotechnics.py

Kept exactly as sqlite holds them (NULL -> null, '' stays '', numbers stay numbers - the conversions are criteria3d_amd/project3d.py's
job, through db_double as loadSoilData's getValue does them):
  * geotechnics: the 18 rows of "SELECT id_class, USCS_code, effective_cohesion, friction_angle FROM geotechnics ORDER BY id_class"
    (loadGeotechnicsParameters, soilDbTools.cpp:38-78);
  * horizons: per soil_code, the (horizon_nr, effective_cohesion, friction_angle) of every horizon ORDER BY horizon_nr - the order and the
    keys of the `horizons` lists of ravone_project.npz's tables_json (loadSoilData, soilDbTools.cpp:283-370).
"""
import json
import sqlite3
from pathlib import Path

DB = Path("/root/reference/DATA/PROJECT/Ravone/SOIL/soil_ER_2021.db")
OUT = Path(__file__).resolve().parent / "ravone_geotechnics.json"


def main():
    db = sqlite3.connect(f"file:{DB}?mode=ro", uri=True)
    geo = [list(r) for r in db.execute("SELECT id_class, USCS_code, effective_cohesion, friction_angle FROM geotechnics ORDER BY id_class")]
    horizons = {}
    for (code,) in db.execute("SELECT DISTINCT soil_code FROM horizons ORDER BY soil_code"):
        rows = db.execute("SELECT horizon_nr, effective_cohesion, friction_angle FROM horizons WHERE soil_code=? ORDER BY horizon_nr", (code,))
        horizons[code] = [list(r) for r in rows]
    OUT.write_text(json.dumps(dict(geotechnics=geo, horizons=horizons), sort_keys=True, separators=(",", ":")) + "\n")
    print(f"{OUT}: {len(geo)} classes, {sum(len(v) for v in horizons.values())} horizons of {len(horizons)} soils")


if __name__ == "__main__":
    main()
