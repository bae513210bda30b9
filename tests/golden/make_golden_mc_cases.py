"""Regenerate tests/golden/mc_cases_classic.npy: scikit-image's CASESCLASSIC table (Lorensen / Bourke's 256 x 16 triangle
table, -1 padded, int8) from its LUT module, so that tests/test_mc_tables.py compares the committed tables with an
independent public copy without needing scikit-image installed.

    python tests/golden/make_golden_mc_cases.py <site-packages>/skimage/measure/_marching_cubes_lewiner_luts.py
"""
import base64
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(lut):
    sp = importlib.util.spec_from_file_location("_mc_luts", lut)
    m = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(m)
    shape, txt = m.CASESCLASSIC
    table = np.frombuffer(base64.decodebytes(txt.encode()), dtype=np.int8).reshape(shape)
    assert table.shape == (256, 16)
    np.save(os.path.join(HERE, "mc_cases_classic.npy"), table)


if __name__ == "__main__":
    main(sys.argv[1])
