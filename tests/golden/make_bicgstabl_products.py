"""Writes tests/golden/bicgstabl_products.json: the products with A that the oracle's BiCGStab restatement (po.bicgstab_ref) and
the BiCGStab(l) restatement (tests/bicgstabl_reference.py) need on the oracle's steady advection-diffusion systems at cell Peclet
number 12.5 (32^2, the disc r = 1 at (2.01, 2.01), rows divided by their diagonal, reltol = 1e-12, zero start), and whether the
BiCGStab(2) count is stable under a one-ulp perturbation of b.  Run from the repository root:
    python tests/golden/make_bicgstabl_products.py"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from oracle import penguin_oracle as po  # noqa: E402
from tests.bicgstabl_reference import bicgstabl_ref, peclet_system  # noqa: E402

RELTOL = 1e-12


def rows():
    out = {}
    for kind in ("rotation", "uniform"):
        A, b = peclet_system(32, kind)
        _, it, _ = po.bicgstab_ref(A, b, reltol=RELTOL, maxiter=50000)
        row = {"n": 32, "unknowns": int(A.shape[0]), "bicgstab": 2 * it}
        for l in (2, 4):
            _, info = bicgstabl_ref(A, b, l=l, reltol=RELTOL)
            row[f"bicgstabl{l}"] = info["products"]
            row[f"bicgstabl{l}_converged"] = bool(info["converged"])
        b1 = b * (1.0 + np.finfo(float).eps * (np.arange(len(b)) % 2))
        _, info1 = bicgstabl_ref(A, b1, l=2, reltol=RELTOL)
        row["bicgstabl2_one_ulp"] = info1["products"]
        out[kind] = row
    return out


if __name__ == "__main__":
    path = Path(__file__).with_name("bicgstabl_products.json")
    path.write_text(json.dumps(rows(), indent=1, sort_keys=True) + "\n")
    print(path.read_text())
