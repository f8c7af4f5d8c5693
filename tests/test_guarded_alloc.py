"""tests/guarded_alloc.py on CPU tensors, and the two lists that keep tests/test_gpu_guard_bands.py complete: every allocating
wrapper of uforecon_amd/ops.py is named by a case or is host-only, and every entry point of include/ufr.h that takes a workspace
byte count has a refusal case.  No GPU."""
import ast
import os
import types

import pytest
import torch

import test_gpu_guard_bands as G
from guarded_alloc import GUARD, PATTERN, GuardedTorch, untouched
from uforecon_amd import _lib

OPS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uforecon_amd", "ops.py")


# ------------------------------------------------------------------------------------------------------------ the helper
def _past(t, n):
    """``t`` with ``n`` more elements behind it (n < 0: in front of it): what a kernel with a wrong bound addresses"""
    if n > 0:
        return t.as_strided((t.numel() + n,), (1,), t.storage_offset())
    return t.as_strided((t.numel() - n,), (1,), t.storage_offset() + n)


def test_all_ones_bytes_are_nan_or_minus_one():
    raw = torch.full((8,), PATTERN, dtype=torch.uint8)
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        assert bool(raw.view(dt).isnan().all()), dt
    for dt in (torch.int8, torch.int16, torch.int32, torch.int64):
        assert bool((raw.view(dt) == -1).all()), dt


def test_an_overrun_and_an_underrun_are_caught_and_named():
    g = GuardedTorch()
    t = g.empty(5, 3, dtype=torch.float32)
    g.check()
    _past(t.view(-1), 1)[-1] = 2.0                          # one element past the end
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "high guard" in msg and "bytes 60 .. 63" in msg and "(5, 3)" in msg and "torch.float32" in msg
    assert "test_guarded_alloc.py" in msg and "test_an_overrun_and_an_underrun" in msg       # the call site
    g = GuardedTorch()
    t = g.zeros(7, dtype=torch.int32)
    _past(t, -2)[0] = 5                                    # two elements before the start
    (r, which, first, last), = g.damage()
    assert (which, first, last) == ("low", -8, -5) and r.shape == (7,) and r.kind == "zeros"      # the four bytes of one int32
    g = GuardedTorch()
    t = g.place(torch.arange(6.0))
    _past(t, 1)[-1] = float("nan")                          # a NaN that is not the pattern is damage too
    assert [d[1] for d in g.damage()] == ["high"]


def test_writes_inside_the_tensor_are_not_flagged():
    g = GuardedTorch()
    ts = [g.empty(4097, dtype=torch.float64), g.empty((3, 5), dtype=torch.uint8), g.zeros((), dtype=torch.float32),
          g.empty(0, 3, dtype=torch.float32), g.full((2, 2), -1, dtype=torch.int32), g.ones(3), g.empty_like(torch.zeros(2, 3))]
    for t in ts:
        t.fill_(1)
    g.check()
    assert g.guarded == len(ts) == len(g.records) and g.placed == 0


def test_fill_policy_and_contents():
    g = GuardedTorch()
    for dt in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        t = g.empty(9, dtype=dt)
        assert bool(t.isnan().all()) and untouched(t), dt           # unwritten memory shows up as NaN
    for dt in (torch.uint8, torch.int32, torch.int64, torch.bool):
        assert not bool(g.empty(9, dtype=dt).any()), dt             # a stale integer must not become a wild index
    assert bool(g.empty_like(torch.zeros(3, dtype=torch.float64)).isnan().all())
    assert not bool(g.empty_like(torch.zeros(3, dtype=torch.int32)).any())
    z = g.zeros(4, 5)
    assert z.dtype == torch.float32 and z.shape == (4, 5) and not bool(z.any())
    assert torch.equal(g.ones((2, 3), dtype=torch.int64), torch.ones(2, 3, dtype=torch.int64))
    f = g.full((3,), float("nan"))
    assert f.dtype == torch.float32 and bool(f.isnan().all())
    assert torch.equal(g.full((2, 2), 255, dtype=torch.uint8), torch.full((2, 2), 255, dtype=torch.uint8))
    assert g.full([4], -1).dtype == torch.int64 and g.full((1,), True).dtype == torch.bool
    src = torch.arange(6, dtype=torch.int32).reshape(2, 3)
    assert torch.equal(g.zeros_like(src), torch.zeros_like(src)) and torch.equal(g.ones_like(src), torch.ones_like(src))
    assert torch.equal(g.full_like(src, 7), torch.full_like(src, 7)) and g.zeros_like(src, dtype=torch.float64).dtype == torch.float64
    p = g.place(src.t())                                            # a copy, contiguous, of a tensor that was not
    assert torch.equal(p, src.t()) and p.is_contiguous() and g.place(None) is None
    g.check()


def test_shapes_as_tuple_list_size_and_varargs():
    g = GuardedTorch()
    for t in (g.empty(2, 3), g.empty((2, 3)), g.empty([2, 3]), g.empty(torch.Size([2, 3])), g.zeros(2, 3), g.zeros((2, 3)),
              g.ones(2, 3), g.ones((2, 3)), g.full((2, 3), 1.5)):
        assert t.shape == (2, 3) and t.is_contiguous() and t.dtype == torch.float32
    assert g.empty(5).shape == (5,) and g.empty(()).shape == () and g.zeros(()).dim() == 0 and g.empty(0).numel() == 0
    g.check()


def test_alignment_class_and_exact_size():
    g = GuardedTorch()
    assert GUARD % 512 == 0
    t = g.empty(3, dtype=torch.float32)
    r = g.records[-1]
    assert r.nbytes == 12 and r.parent.numel() == 2 * GUARD + 12                 # not rounded up
    assert t.data_ptr() == r.parent.data_ptr() + GUARD                          # the parent's alignment, shifted by whole granules
    with pytest.raises(AssertionError):
        GuardedTorch(guard=100)


def test_a_module_runs_on_the_proxy(monkeypatch):
    """the swap the GPU test makes, on a stand-in module: forwarded attributes keep isinstance and dtypes working, the
    allocation is guarded, and the patch ends with the test's monkeypatch"""
    m = types.ModuleType("wrapper_like")
    m.torch = torch
    exec("def make(n):\n    out = torch.empty(n, dtype=torch.float32)\n    assert isinstance(out, torch.Tensor)\n"
         "    with torch.no_grad():\n        out.copy_(torch.arange(n, dtype=torch.float32))\n    return out\n", m.__dict__)
    g = GuardedTorch().install(monkeypatch, m)
    out = m.make(5)
    assert g.guarded == 1 and torch.equal(out, torch.arange(5.0)) and g.records[0].site.startswith("<string>:2 (make)")
    g.check()
    snap = g.snapshot()
    assert g.changed(snap) == []
    out.view(torch.int32)[2] = -1                            # all four bytes of one element
    assert len(g.changed(snap)) == 1 and "bytes 8 .. 11" in g.changed(snap)[0]


# ------------------------------------------------------------------------------------------------------------ coverage
ALLOCATORS = {"empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like"}

# public names of ops.py that the walk below finds and that launch NO kernel on what they allocate.  Nothing else may stand here.
# (The host tables -- grid_tables, marching_cubes_table, smooth_factors, mask_half_widths -- call none of the guarded allocators
# and no size query, so the walk does not find them and they need no entry.)
EXEMPT = {
    "poisson_workspace_bytes": "a size query handed on: allocates nothing, launches nothing",
    "conv3d_planes_supported": "a size query compared with 0: allocates nothing, launches nothing",
}


def _allocates(node) -> bool:
    for n in ast.walk(node):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute):
            if n.func.attr in ALLOCATORS and isinstance(n.func.value, ast.Name) and n.func.value.id == "torch":
                return True
            if n.func.attr.endswith("_workspace_bytes"):
                return True
    return False


def allocating_wrappers(path=OPS):
    """The public names of ops.py whose body calls a guarded allocator or a ``*_workspace_bytes`` query: top-level functions by
    name, a public class by its name when its ``__init__`` does (constructing it is the call), and every other public method that
    does as ``Class.method`` -- a case must name and call that method, constructing the class does not cover it"""
    tree = ast.parse(open(path).read())
    names = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and not node.name.startswith("_") and _allocates(node):
            names.append(node.name)
        elif isinstance(node, ast.ClassDef) and not node.name.startswith("_"):
            for m in node.body:
                if isinstance(m, ast.FunctionDef) and _allocates(m):
                    if m.name == "__init__":
                        names.append(node.name)
                    elif not m.name.startswith("_"):
                        names.append(f"{node.name}.{m.name}")
    return names


def test_the_walk_names_allocating_methods(tmp_path):
    src = tmp_path / "like_ops.py"
    src.write_text("import torch\nclass A:\n    def __init__(self):\n        self.t = torch.empty(3)\n    def grow(self):\n"
                   "        return torch.zeros(4)\n    def _hidden(self):\n        return torch.ones(2)\n    def plain(self):\n"
                   "        return 1\nclass _B:\n    def f(self):\n        return torch.empty(1)\ndef g(lib):\n"
                   "    return lib.ufr_x_workspace_bytes(3)\ndef _h():\n    return torch.empty(1)\ndef k(x):\n    return x.new_zeros(3)\n")
    assert allocating_wrappers(str(src)) == ["A", "A.grow", "g"]


def test_every_allocating_wrapper_of_ops_is_in_the_table_or_host_only():
    names = allocating_wrappers()
    assert len(names) > 75 and {"render_rays", "FrameHandle", "select_rays", "mesh_simplify"} <= set(names)    # the walk works
    covered = {n for c in G.CASES.values() for n in c.covers}
    missing = [n for n in names if n not in covered and n not in EXEMPT]
    assert not missing, f"allocating wrappers of ops.py without a guard-band case: {missing}"
    both = sorted(set(EXEMPT) & covered)
    assert not both, both
    stale = [n for n in EXEMPT if n not in names]
    assert not stale, f"EXEMPT names something that does not allocate (or is gone): {stale}"
    assert all(isinstance(r, str) and r for r in EXEMPT.values())


def test_cases_name_real_wrappers_and_modules():
    import importlib

    for c in G.CASES.values():
        assert c.allocs >= 1 and c.covers, c.name
        for n in c.covers:
            mod, _, attr = n.rpartition(".")
            if mod and mod not in G.MODULES:                        # "Class.method" of ops.py
                m, mod = getattr(importlib.import_module("uforecon_amd.ops"), mod), ""
            else:
                m = importlib.import_module("uforecon_amd." + (mod or "ops"))
            assert hasattr(m, attr), (c.name, n)
        assert set(c.modules) <= set(G.MODULES), c.name
        mods = {(n.rpartition(".")[0] if n.rpartition(".")[0] in G.MODULES else "") or "ops" for n in c.covers}
        assert mods <= set(c.modules), (c.name, mods)               # a module whose wrapper is covered is patched


def test_every_entry_point_with_a_workspace_count_has_a_refusal_case():
    entries = G.workspace_entry_points()
    assert len(entries) >= 30 and entries["ufr_frame_prepare"] == 2 and entries["ufr_select_rays"] == 5
    assert entries["ufr_render_rays"] is None and entries["ufr_render_rays_pair"] is None
    for name, index in entries.items():                             # the header and the ctypes binding agree on the position
        args = _lib.SIGNATURES[name][1]
        assert index is None or args[index] is _lib.sz, (name, index)
    missing = sorted(set(entries) - set(G.REFUSALS))
    assert not missing, f"entry points with a workspace byte count and no refusal case: {missing}"
    unknown = sorted(set(G.REFUSALS) - set(entries))
    assert not unknown, unknown
