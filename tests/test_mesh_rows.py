"""The host side of the per-vertex mesh stages, checked without a GPU: ops._corner_runs (the one stable sort of the corner
slots) against denoise_ref.sorted_rows, exactly, and the messages of ops._faces.  What the kernels do with the order is in
test_gpu_raster.py, test_gpu_color_mesh.py, test_gpu_smooth_mesh.py and test_gpu_denoise_mesh.py."""
import numpy as np
import pytest
import torch

import denoise_ref as D
import simplify_ref as S
from uforecon_amd import ops
from uforecon_amd._lib import UfrError


def _cases():
    for V, F in ((1, 1), (3, 257), (257, 1), (64, 256)):
        yield f"soup {V}x{F}", V, S.soup(V, F)[1]
    yield "a vertex named twice by one face", 5, np.array([[0, 1, 2], [3, 3, 1], [2, 3, 4], [1, 1, 1]], np.int32)
    yield "the last vertices unreferenced", 9, np.array([[0, 1, 2], [2, 1, 3], [0, 3, 1]], np.int32)


@pytest.mark.parametrize("name,V,faces", list(_cases()), ids=[c[0] for c in _cases()])
def test_corner_runs_equal_the_reference_order(name, V, faces):
    slots, runs = ops._corner_runs(torch.from_numpy(faces), V)
    want_slots, want_runs = D.sorted_rows(V, faces)
    assert slots.dtype == runs.dtype == torch.int64 and slots.is_contiguous() and runs.is_contiguous()
    assert slots.device.type == runs.device.type == "cpu"
    assert tuple(slots.shape) == (3 * len(faces),) and tuple(runs.shape) == (V + 1,)
    assert np.array_equal(slots.numpy(), want_slots.astype(np.int64))
    assert np.array_equal(runs.numpy(), want_runs.astype(np.int64))
    assert int(runs[0]) == 0 and int(runs[-1]) == 3 * len(faces)          # every corner stands in exactly one run


def test_corner_runs_stay_int64_without_faces():
    slots, runs = ops._corner_runs(torch.zeros((0, 3), dtype=torch.int32), 4)
    assert slots.dtype == runs.dtype == torch.int64 and tuple(slots.shape) == (0,) and runs.tolist() == [0] * 5


def test_faces_checks_keep_their_messages():
    good = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    assert ops._faces(good, 4, "who") == 2 and ops._faces(good, 4, "who", rows=True) == 2
    assert ops._faces(torch.zeros((0, 3), dtype=torch.int32), 0, "who") == 0
    with pytest.raises(UfrError, match=r"^faces: expected shape \(F, 3\), got \(2, 4\)$"):
        ops._faces(torch.zeros((2, 4), dtype=torch.int32), 4, "who")
    with pytest.raises(UfrError, match=r"^faces: expected shape \(F, 3\), got \(6,\)$"):
        ops._faces(good.reshape(-1), 4, "who")
    with pytest.raises(UfrError, match=r"^faces: dtype torch\.int64, expected torch\.int32$"):
        ops._faces(good.to(torch.int64), 4, "who")
    low = good.clone()
    low[1, 2] = -1
    with pytest.raises(UfrError, match=r"^who: face indices span -1\.\.2, the mesh has 4 vertices$"):
        ops._faces(low, 4, "who")
    with pytest.raises(UfrError, match=r"^who: face indices span 0\.\.3, the mesh has 3 vertices$"):        # an index of V
        ops._faces(good, 3, "who")
    with pytest.raises(UfrError, match=r"^who: face indices span 0\.\.3, the mesh has 0 vertices$"):
        ops._faces(good, 0, "who")


def test_block_and_chunk_have_one_value():
    assert ops.SMOOTH_BLOCK == ops.DENOISE_BLOCK == ops.MESH_ROW_BLOCK == 256
    assert ops.SMOOTH_CHUNK == ops.DENOISE_CHUNK == ops.MESH_ROW_CHUNK == 1024
    from uforecon_amd.build import SOURCES

    assert "api_mesh.hip" in SOURCES and "api_geometry.hip" in SOURCES
