"""Generates tests/golden/glue_ref.npz from oracle/_ref (the reference's own reference_path_smoother.cpp and path_optimizer.cpp compiled through oracle/ref_shim; only
where the reference tree exists): segmentRawReference and the first half of segmentSmoothedPath on the inputs of tests/test_glue_edges.py (raw_inputs, init_inputs).
Data only: the inputs as recorded (the test checks that it still builds the same ones) and the station lists, flags, initial errors and trimmed lengths."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_glue_edges as T  # noqa: E402

if __name__ == "__main__":
    from oracle import ref_py

    out = dict(T.reference_stages(ref_py))
    raw, inp = T.raw_inputs(), T.init_inputs()
    for k in ("knot_s", "knot_x", "knot_y"):
        out["in_raw_" + k] = raw["sp"][k]
        out["in_init_" + k] = inp["sp"][k]
    out.update(in_init_start=inp["start"], in_init_goal=inp["goal"], in_init_length=inp["length"])
    print("raw n", out["raw_n"], "init rows", out["init_rows"], "ok", out["init_ok"], "length", out["init_init"][:, 2])
    np.savez_compressed(os.path.join(HERE, "glue_ref.npz"), **out)
