"""What the loaders share since uforecon_amd/cameras.py and host_forms.py exist: the one camera-file parser against the four
forms it replaced, the one pair-file reader, and the one float64 ray table against the two functions it replaced.  Every
comparison is for equality: the goldens pin these bits."""
import numpy as np
import pytest
import torch

import dtu_scan_golden as G
import dtu_train_golden as T
import general_scan_golden as S
from uforecon_amd import cameras, clean_mesh, depth_fusion, dtu_scan, dtu_train, general_scan, host_forms


def _cam_texts():
    """the camera files of the DTU scan, training and custom-scene fixtures"""
    texts = [str(v) for g in (G.golden(), T.golden()) for k, v in g.items() if k.startswith("cam/")]
    texts += [str(v) for k, v in S.golden().items() if k.startswith("file/cams/") and k.endswith("_cam.txt") and not str(v).startswith("@")]
    return texts


def _k4(K):
    K4 = np.float32(np.diag([1, 1, 1, 1]))
    K4[:3, :3] = K
    return K4


def test_one_cam_file_parser_equals_the_four_forms_it_replaced(tmp_path):
    texts = _cam_texts()
    assert len(texts) >= 49 + 3 + 5 and len({t.splitlines()[11] for t in texts}) > 3
    for n, text in enumerate(texts):
        path = tmp_path / ("%d_cam.txt" % n)
        path.write_text(text)
        lines = [line.rstrip() for line in text.splitlines()]
        E = np.fromstring(" ".join(lines[1:5]), dtype=np.float32, sep=" ").reshape((4, 4))          # the three loaders' parse
        K = np.fromstring(" ".join(lines[7:10]), dtype=np.float32, sep=" ").reshape((3, 3))
        E_split = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)           # clean_mesh's
        K_split = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
        tokens = lines[11].split()
        depth_min, interval = float(tokens[0]), float(tokens[1])
        k, e, depth = cameras.read_cam_file(path)
        scan, train, general = dtu_scan.read_cam_file(path), dtu_train.read_cam_file(path), general_scan.read_cam_file(path)
        mesh = clean_mesh.read_cam_file(path)
        same = lambda a, b: a.dtype == b.dtype == np.float32 and np.array_equal(a, b)  # noqa: E731
        assert same(k, K) and same(e, E) and same(k, K_split) and same(e, E_split) and depth == [float(t) for t in tokens]
        P = _k4(K) @ E
        # dtu_test_sparse.py: (P, depth_min, interval * 1.06)
        assert same(scan[0], P) and scan[1:] == (depth_min, interval * 1.06)
        # dtu_train.py: (K4, E, [depth_min, depth_max], depth_min, interval * 1.06), depth_max = min + interval * 192
        assert same(train[0], _k4(K)) and same(train[1], E) and train[2:] == ([depth_min, depth_min + interval * 192], depth_min, interval * 1.06)
        # general_fit.py: near = the first token, far = the last
        assert same(general[0], P) and general[1:] == (depth_min, float(tokens[-1]), depth_min, interval * 1.06)
        # clean_mesh: (K, E), and the one place that forms K4 @ E
        assert same(mesh[0], K_split) and same(mesh[1], E_split) and same(clean_mesh.projection(*mesh), P)


def test_pair_file_entry_without_sources(tmp_path):
    p = tmp_path / "pair.txt"
    p.write_text("4\n0\n3 1 0.5 2 0.4 3 0.3\n1\n0\n2\n1 0 9.0\n3\n10 0 1 1 1 2 1 0 1 1 1 2 1 0 1 1 1 2 1 3 1\n")
    every = [(0, [1, 2, 3]), (1, []), (2, [0]), (3, [0, 1, 2, 0, 1, 2, 0, 1, 2, 3])]
    assert cameras.read_pair_file(str(p)) == every                                        # the loaders' form keeps it
    assert depth_fusion.read_pair_file(str(p)) == [e for e in every if e[0] != 1]          # depth fusion drops it


def _parent_pixel_rays_host(m_inv, H, W, origin, hp):
    """dtu_scan.pixel_rays_host before the two functions became one"""
    m = torch.as_tensor(m_inv, dtype=torch.float32)
    v = torch.from_numpy(np.matmul(m.numpy(), hp))[:3]
    if origin is not None:
        v = v - torch.as_tensor(origin, dtype=torch.float32)[:, None]
    return (v / torch.norm(v, dim=0)).float()


def _parent_rays64(m_inv, origin, hp):
    """DtuTrain._rays64 before the two functions became one"""
    v = torch.from_numpy(np.matmul(torch.as_tensor(m_inv, dtype=torch.float32).numpy(), hp))[:3]
    if origin is not None:
        v = v - torch.as_tensor(origin, dtype=torch.float32)[:, None]
    return v / torch.linalg.norm(v, dim=0, keepdim=True)


@pytest.mark.parametrize("H,W", [(5, 7), (32, 64)])
@pytest.mark.parametrize("with_origin", [False, True])
def test_one_ray_table_equals_the_two_it_replaced(H, W, with_origin):
    rng = np.random.default_rng(H * 2 + with_origin)
    hp = cameras.homo_pixels(H, W)
    for scale in (1.0, 300.0):
        m = torch.from_numpy((rng.normal(size=(4, 4)) * scale).astype(np.float32))
        origin = torch.from_numpy(rng.normal(size=3).astype(np.float32)) if with_origin else None
        t64 = host_forms.pixel_rays64(m, hp, origin)
        want64 = _parent_rays64(m, origin, hp)
        assert t64.dtype == want64.dtype == torch.float64 and t64.shape == (3, H * W) and torch.equal(t64, want64)   # cam_ray_d.z
        want32 = _parent_pixel_rays_host(m, H, W, origin, hp)
        for got in (host_forms.pixel_rays_host(m, H, W, origin, hp), host_forms.pixel_rays_host(m, H, W, origin),
                    host_forms.pixel_rays("cpu", m, H, W, origin, hp)):
            assert got.dtype == torch.float32 and torch.equal(got, want32) and torch.equal(got, want64.float())
