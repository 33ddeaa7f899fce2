"""Writes tests/golden/resample_pil.npz: what Pillow's BILINEAR resize (the Resize of the reference's datasets, src/dataset/dtu.py:70-72)
makes of the seeded inputs of tests/resample_ref.py, one `<tag>` array (Hout,Wout,3) uint8 per shape, and the Pillow version that wrote
them.  The inputs are regenerated from their seeds by the tests, so the fixture holds outputs only.  Run from the repository root:
    python tests/golden/make_resample_golden.py"""
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_ref as RR                                       # noqa: E402

if __name__ == '__main__':
    out = {tag: RR.pil_resize(RR.make_input(tag), size) for tag, (_, size) in RR.SHAPES.items()}
    out['pillow_version'] = np.array(PIL.__version__)
    np.savez_compressed(RR.GOLDEN, **out)
    print(RR.GOLDEN, os.path.getsize(RR.GOLDEN), 'bytes, Pillow', PIL.__version__)
