"""The down_up golden cases (tests/golden/make_golden.py): the reference's outputs are stored, their inputs are not -- they are
the seeded draws the generator made, in the order of `down_up_meta`, and are drawn again here.  Each stored SHA-256 pins the
redrawn input to the exact bytes the reference saw, so a changed random stream fails instead of testing other data."""
import hashlib
import json
import os

import numpy as np

DOWN_UP_SEED = 20250929


def down_up_cases(golden_dir):
    """[(meta, input, reference output)] of every case in lp_misc.json's down_up_meta, inputs float32."""
    with open(os.path.join(golden_dir, "lp_misc.json")) as f:
        meta = json.load(f)["down_up_meta"]
    vec = np.load(os.path.join(golden_dir, "down_up_vectors.npz"))
    rng = np.random.default_rng(DOWN_UP_SEED)
    cases = []
    for m in meta:
        x = rng.standard_normal(tuple(m["shape"])).astype(np.float32)
        assert hashlib.sha256(x.tobytes()).hexdigest() == str(vec[m["name"] + "_in_sha256"]), (
            "%s: the seeded input no longer matches the one the golden output was made from" % m["name"])
        cases.append((m, x, vec[m["name"] + "_out"]))
    return cases
