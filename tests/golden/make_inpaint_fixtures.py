#!/usr/bin/env python3
"""Convert the reference's 2 content-aware fill goldens (``tests/golden/inpaint/<name>.png``, written by ``assert_golden`` for ``tests/inpaint.rs``)
into one raw-RGBA fixture file.  Pixels only: every entry of ``inpaint.npz`` is a ``(64, 64, 4) uint8`` array keyed ``"inpaint/<name>"``.
Run where the reference checkout exists; the tests only read the result.

    python tests/golden/make_inpaint_fixtures.py <reference checkout>     (or PFX_REFERENCE=<reference checkout>)
"""
import os
import sys

import numpy as np
from PIL import Image


def main() -> int:
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PFX_REFERENCE")
    if not ref:
        print(__doc__)
        return 2
    d = os.path.join(ref, "tests", "golden", "inpaint")
    out = {}
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".png"):
            out[f"inpaint/{fn[:-4]}"] = np.asarray(Image.open(os.path.join(d, fn)).convert("RGBA"), dtype=np.uint8).copy()
    assert len(out) == 2 and all(v.shape == (64, 64, 4) for v in out.values())
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "inpaint.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out)} images, {os.path.getsize(dst)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
