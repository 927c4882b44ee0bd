"""Writes tests/golden/idrs_products.json: the products with A that the IDR(s) restatement (tests/idrs_reference.py) needs on the
oracle's steady advection-diffusion systems at cell Peclet number 12.5 (32^2, the disc r = 1 at (2.01, 2.01), rows divided by
their diagonal, reltol = 1e-12, zero start) for s = 1, 2, 4, 8, next to the BiCGStab and BiCGStab(l) counts of
tests/golden/bicgstabl_products.json, and the same counts under a one-ulp perturbation of b.  Run from the repository root:
    python tests/golden/make_idrs_products.py"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from tests.idrs_reference import idrs_ref, peclet_system  # noqa: E402

RELTOL = 1e-12
SHADOWS = (1, 2, 4, 8)


def rows():
    other = json.loads(Path(__file__).with_name("bicgstabl_products.json").read_text())
    out = {}
    for kind in ("rotation", "uniform"):
        A, b = peclet_system(32, kind)
        row = {"n": 32, "unknowns": int(A.shape[0]), "bicgstab": other[kind]["bicgstab"], "bicgstabl2": other[kind]["bicgstabl2"],
               "bicgstabl4": other[kind]["bicgstabl4"]}
        b1 = b * (1.0 + np.finfo(float).eps * (np.arange(len(b)) % 2))
        for s in SHADOWS:
            _, info = idrs_ref(A, b, s=s, reltol=RELTOL)
            _, info1 = idrs_ref(A, b1, s=s, reltol=RELTOL)
            row[f"idrs{s}"] = info["products"]
            row[f"idrs{s}_converged"] = bool(info["converged"])
            row[f"idrs{s}_restarts"] = info["restarts"]
            row[f"idrs{s}_one_ulp"] = info1["products"]
            row[f"idrs{s}_one_ulp_converged"] = bool(info1["converged"])
        out[kind] = row
    return out


if __name__ == "__main__":
    path = Path(__file__).with_name("idrs_products.json")
    path.write_text(json.dumps(rows(), indent=1, sort_keys=True) + "\n")
    print(path.read_text())
