#!/usr/bin/env python3
"""Golden vector for the C-index: the reference's own pure-Python CIndex (MICCAI-2022/utils.py:409-421), compiled from the
file where it lies (the module imports lifelines / imblearn, absent here), on a TIE-FREE risk / time vector - the case in
which it equals the lifelines rule of CIndex_lifeline (utils.py:424-425).  Writes tests/golden/cindex_tiefree.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def main():
    src = open("/root/reference/MICCAI-2022/utils.py").read()
    s0 = src.index("def CIndex("); s1 = src.index("def CIndex_lifeline(", s0)
    ns = {"np": np}
    exec(compile(src[s0:s1], "CIndex<reference>", "exec"), ns)
    rs = np.random.RandomState(11)
    N = 200
    hazards = rs.permutation(N).astype(np.float32) / N + rs.rand(N).astype(np.float32) * 1e-3   # distinct
    survtime = (rs.permutation(N) + 1).astype(np.float32) * 3.0                                   # distinct
    labels = (rs.rand(N) > 0.35).astype(np.float32)
    assert len(np.unique(hazards)) == N and len(np.unique(survtime)) == N
    cidx = ns["CIndex"](hazards, labels, survtime)
    np.savez_compressed(os.path.join(HERE, "cindex_tiefree.npz"), hazards=hazards, survtime=survtime, labels=labels,
                        cindex=np.float64(cidx))
    print("wrote cindex_tiefree.npz", cidx)


if __name__ == "__main__":
    main()
