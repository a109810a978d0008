"""Records the REFERENCE's own ``_random_edge_index(n, r, seed)`` (its ``03_build_graphs.py:57-78``) at small node counts into
tests/golden/random_ragged.npz.

    PYTHONDONTWRITEBYTECODE=1 python tests/gen_random_ragged_golden.py <directory of the reference>

The reference's ``03_build_graphs.py`` is imported from where it lies (nothing of it is copied here).  The fixture holds only
outputs: one int16 ``[2, E]`` array per (n, r, seed) of ``rand_graph_ragged_ref.GOLDEN_CASES`` under the key ``n<n>.r<r>.s<seed>``, r as given
(the reference clamps it).  The node counts are those a lesion-only frame has and the 196-node goldens of
tests/golden/graphs.npz do not cover: no word consumed (2), one word per node (3), a complete graph under the clamp (5), the
first state regeneration (27), two bitmap words (33), more nodes than a wave has lanes (65).  Run once; the tests never run it.
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rand_graph_ragged_ref import GOLDEN, GOLDEN_CASES, golden_key  # noqa: E402


def load_reference_build_graphs(ref_dir):
    spec = importlib.util.spec_from_file_location("reference_build_graphs", os.path.join(ref_dir, "03_build_graphs.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
    except (FileNotFoundError, OSError):      # its module-level driver lists a directory of its authors' cluster, after the
        pass                                  # functions are defined (oracle/gen_golden.py loads it the same way)
    return mod


def main():
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    ref = load_reference_build_graphs(sys.argv[1])
    out = {}
    for n, r, s in GOLDEN_CASES:
        e = ref._random_edge_index(n, r=r, seed=s).numpy()
        assert e.shape[0] == 2 and (e.size == 0 or (0 <= e.min() and e.max() < n))
        out[golden_key(n, r, s)] = e.astype(np.int16)
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN}: {len(out)} arrays, {os.path.getsize(GOLDEN)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
