#!/usr/bin/env python3
"""Convert the reference's 20 shape goldens (``tests/golden/shapes/<name>.png``, written by ``assert_golden`` for
``tests/visual_shapes.rs``) into one raw-RGBA fixture file.  Pixels only: every entry of ``shapes.npz`` is a
``(128, 128, 4) uint8`` array keyed ``"shapes/<name>"``.  Run where the reference checkout exists; the tests only read the result.

    python tests/golden/make_shape_fixtures.py <reference checkout>     (or PFX_REFERENCE=<reference checkout>)
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
    d = os.path.join(ref, "tests", "golden", "shapes")
    out = {}
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".png"):
            out[f"shapes/{fn[:-4]}"] = np.asarray(Image.open(os.path.join(d, fn)).convert("RGBA"), dtype=np.uint8).copy()
    assert len(out) == 20 and all(v.shape == (128, 128, 4) for v in out.values())
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shapes.npz")
    np.savez_compressed(dst, **out)
    print(f"wrote {dst}: {len(out)} images, {os.path.getsize(dst)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
