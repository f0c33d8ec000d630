"""Child of test_gpu_attn_paths.test_backward_forced_windows_per_block.

    python tests/_attn_wpb_child.py B H W HEADS WS SHIFT V_BIAS WPB OUT.npz

Started with MDE_ATTN_BWD_WPB=WPB in its environment (the library reads it once
per process).  Runs the case's forward, then its backward inside guarded_abi()
(tests/_abi_guard.py: guard bands around every buffer and the slab, two runs
from poisoned outputs and scratch), checks that the workspace query shows the
forced grouping, and writes the five gradients to OUT.npz.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def main(argv):
    b, h, w, heads, ws, shift, v_bias, wpb = (int(a) for a in argv[:8])
    out = argv[8]
    assert os.environ.get("MDE_ATTN_BWD_WPB") == str(wpb), os.environ.get("MDE_ATTN_BWD_WPB")
    import numpy as np

    from tests import _attn_cases as ac
    nwin, nblk = ac.backward_blocks(b, h, w, heads, ws)
    assert nblk == -(-nwin // wpb), f"{nwin} windows at {wpb} per block, but {nblk} blocks"
    res = ac.run_kernel(b, h, w, heads, ws, shift, bool(v_bias), guard_backward=True)
    np.savez(out, **{k: res[k].numpy() for k in ac.GRADS if res[k] is not None})
    print(f"OK nwin {nwin} nblk {nblk} wpb {wpb}")


if __name__ == "__main__":
    main(sys.argv[1:])
