#!/usr/bin/env python3
"""Generate tests/golden/ravone_crops.json: the rows of the `crop` table of DATA/crop_Ravone.db of the Ravone project (BASELINE config 5)
that its land units name (land_units.id_crop of ravone_project.npz), as data.  Run by hand where the reference's database lies (it is
read read-only); no test calls it:

    python tests/golden/make_ravone_crops.py --reference <CRITERIA3D tree>

Kept exactly as sqlite holds them (NULL -> null, '' stays '', numbers stay numbers - the conversions of loadCropParameters are
criteria3d_amd/project3d.py's job): {"columns": [...], "crop": [{column: value}, ...]} ordered by id_crop.
"""
import argparse
import json
import sqlite3
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
OUT = HERE / "ravone_crops.json"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the CRITERIA3D tree (DATA/PROJECT/Ravone)")
    a = ap.parse_args()
    tables = json.loads(str(np.load(HERE / "ravone_project.npz")["tables_json"]))
    ids = sorted({r[4] for r in tables["land_units"] if r[4]})
    db = sqlite3.connect(f"file:{Path(a.reference) / 'DATA' / 'PROJECT' / 'Ravone' / 'DATA' / 'crop_Ravone.db'}?mode=ro", uri=True)
    cur = db.execute(f"SELECT * FROM crop WHERE id_crop IN ({','.join('?' * len(ids))}) ORDER BY id_crop", ids)
    cols = [d[0] for d in cur.description]
    rows = [dict(zip(cols, r)) for r in cur]
    OUT.write_text(json.dumps(dict(columns=cols, crop=rows), separators=(",", ":")) + "\n")
    print(f"{OUT}: {len(rows)} crops of {len(ids)} ids ({', '.join(ids)})")


if __name__ == "__main__":
    main()
