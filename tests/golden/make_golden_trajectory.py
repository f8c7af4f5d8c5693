"""Records the reference's own ``interpolate_trajectory`` (render_trajectory_dtu.py:57-77) into trajectory_slerp.npz.

    python tests/golden/make_golden_trajectory.py /path/to/reference

Run where the reference tree and scipy are at hand; the tests read only the .npz.  The script cannot be imported (its top level
runs the whole job), so the one function is cut out of its text with ``ast``, in memory, and given what it names: numpy, torch,
scipy's ``Rotation``, ``Slerp`` and ``interp1d``.  Nothing of the reference is written anywhere.

Keys are float64 and orthonormal to rounding (float32-derived keys are deliberately not pinned: the reference's result then
moves with the key's own departure from a rotation).  Cases: K = 2, 3, 5 keys; K = 3 with key 2 equal to key 0 (the reference's
own [23, 24, 23] call) and with key 1 equal to key 0; relative rotations of about 1e-5, 0.3, 1.5 and 3.0 rad; 240 and 7 frames.
"""
import ast
import os
import sys

import numpy as np


def reference_function(ref_root):
    import torch
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp

    path = os.path.join(ref_root, "render_trajectory_dtu.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "interpolate_trajectory"]
    assert len(fn) == 1
    ns = {"np": np, "torch": torch, "Rotation": Rotation, "Slerp": Slerp, "interp1d": interp1d}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return lambda w2cs, n: ns["interpolate_trajectory"](torch.from_numpy(np.asarray(w2cs, np.float64)), num_views=n).numpy()


def keys(rng, angles, repeat=None):
    """w2cs (len(angles)+1,4,4) float64: key k+1 is key k turned by angles[k] about a random axis and moved; ``repeat`` (i, j)
    makes key i a copy of key j"""
    from scipy.spatial.transform import Rotation

    R = Rotation.random(random_state=int(rng.integers(1 << 30)))
    c2ws = []
    pos = rng.uniform(-400, 400, 3)
    for a in [None] + list(angles):
        if a is not None:
            axis = rng.normal(size=3)
            R = R * Rotation.from_rotvec(a * axis / np.linalg.norm(axis))
            pos = pos + rng.uniform(-60, 60, 3)
        c = np.eye(4)
        c[:3, :3], c[:3, 3] = R.as_matrix(), pos
        c2ws.append(c)
    if repeat is not None:
        c2ws[repeat[0]] = c2ws[repeat[1]].copy()
    return np.linalg.inv(np.stack(c2ws))


CASES = [("k2_tiny", [1e-5], None), ("k2_03", [0.3], None), ("k2_15", [1.5], None), ("k2_30", [3.0], None),
         ("k3_mixed", [0.3, 1.5], None), ("k3_loop", [1.5, 0.7], (2, 0)), ("k3_equal_neighbours", [0.9, 0.3], (1, 0)),
         ("k5_all", [1e-5, 0.3, 1.5, 3.0], None)]
NUM_VIEWS = (240, 7)


def main(ref_root):
    ref = reference_function(ref_root)
    rng = np.random.default_rng(20240607)
    out = {"names": np.array([c[0] for c in CASES]), "num_views": np.array(NUM_VIEWS)}
    for name, angles, repeat in CASES:
        w2cs = keys(rng, angles, repeat)
        out[f"{name}_w2cs"] = w2cs
        for n in NUM_VIEWS:
            out[f"{name}_c2ws_{n}"] = ref(w2cs, n)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "trajectory_slerp.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
