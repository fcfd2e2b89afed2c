"""Generate tests/golden/variable.npz from the reference's own CPU zfp 0.5.0
(oracle/_ref/libzfp_ref.so) -- TEST INFRASTRUCTURE.

    python tests/golden/make_variable_golden.py

Per case of tests/test_variable.py `cases()` (shape, type, fixed precision or
fixed accuracy, parameter): the SHA-256 of zfp_compress's stream, the uint16
block lengths, the total bit count and the SHA-256 of zfp_decompress's array.
Data only; the inputs are the seeded recipe of tests/test_variable.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import test_variable as tv  # noqa: E402


def main() -> None:
    if oracle.reference is None:
        raise SystemExit("oracle/_ref/libzfp_ref.so is not built")
    np.savez_compressed(tv.FIXTURE, **tv.generate(oracle.reference))
    print(tv.FIXTURE, os.path.getsize(tv.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
