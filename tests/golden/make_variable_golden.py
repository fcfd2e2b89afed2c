"""Generate tests/golden/variable.npz and tests/golden/variable_paths.npz from
the reference's own CPU zfp 0.5.0 (oracle/_ref/libzfp_ref.so) -- TEST
INFRASTRUCTURE.

    python tests/golden/make_variable_golden.py

variable.npz, per case of tests/test_variable.py `cases()` (shape, type, fixed
precision or fixed accuracy, parameter): the SHA-256 of zfp_compress's stream,
the uint16 block lengths, the total bit count and the SHA-256 of
zfp_decompress's array.  variable_paths.npz, per case of
tests/test_variable_paths.py `cases()` (the block zoo at every precision and a
ladder of tolerances, arrays of several scan tiles, arrays whose waves end on
stream words): the same with the lengths as a SHA-256 too.  Data only; the
inputs are the seeded recipes of those two modules and of tests/block_zoo.py.
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
import test_variable_paths as tp  # noqa: E402


def main() -> None:
    if oracle.reference is None:
        raise SystemExit("oracle/_ref/libzfp_ref.so is not built")
    for mod in (tv, tp):
        np.savez_compressed(mod.FIXTURE, **mod.generate(oracle.reference))
        print(mod.FIXTURE, os.path.getsize(mod.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
