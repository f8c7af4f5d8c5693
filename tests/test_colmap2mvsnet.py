"""The COLMAP converter (uforecon_amd/colmap2mvsnet.py) on the host: its binary reader, its file texts and its scores against
what the reference's own colmap2mvsnet.py wrote for the same model (tests/golden/colmap_small.npz; what that pins and what it
does not is in tests/golden/make_golden_colmap.py), and its one-line exits."""
import ast
import os
import shutil

import numpy as np
import pytest

import general_scan_golden as S
from uforecon_amd import colmap2mvsnet as C

RUNS = {"default": {}, "max_d": {"max_d": 64, "interval_scale": 2.0}}
SCORE_ATOL = 5e-7          # what the pair file's %f carries


def golden():
    return S.golden("colmap_small")


@pytest.fixture()
def dense(tmp_path):
    return S.write_colmap_scene(tmp_path)


def _small_model():
    rng = np.random.default_rng(8)
    cameras = {1: C.Camera(1, "SIMPLE_PINHOLE", 64, 48, np.array([70.0, 32.0, 24.0])),
               7: C.Camera(7, "OPENCV", 64, 48, np.array([71.0, 72.0, 31.0, 23.0, 0.1, 0.01, 0.001, 0.002]))}
    images, points = {}, {}
    for k in (1, 2, 3):
        n = (5, 0, 3)[k - 1]
        images[k] = C.Image(k, rng.normal(size=4), rng.normal(size=3), (1, 7, 1)[k - 1], "a %d.png" % k, rng.uniform(0, 64, (n, 2)),
                            np.array([4, -1, 9, 9, 2 ** 40][:n], np.int64))
    for p in (4, 9, 2 ** 40):
        t = (2, 0, 3)[(4, 9, 2 ** 40).index(p)]
        points[p] = C.Point3D(p, rng.normal(size=3), rng.integers(0, 256, 3), 0.5, np.arange(1, t + 1, dtype=np.int32),
                              np.arange(t, dtype=np.int32))
    return cameras, images, points


def test_binary_reader_round_trips_a_model(tmp_path):
    cameras, images, points = _small_model()
    C.write_model(str(tmp_path / "m"), cameras, images, points)
    assert os.path.getsize(tmp_path / "m" / "cameras.bin") == 8 + (24 + 3 * 8) + (24 + 8 * 8)
    assert os.path.getsize(tmp_path / "m" / "images.bin") == 8 + 3 * (64 + 8 + 8) + 8 * 24          # names of 7 bytes and a zero
    assert os.path.getsize(tmp_path / "m" / "points3D.bin") == 8 + 3 * 51 + 5 * 8
    c2, i2, p2 = C.read_model(str(tmp_path / "m"))
    assert list(c2) == [1, 7] and list(i2) == [1, 2, 3] and list(p2) == [4, 9, 2 ** 40]
    for k, c in cameras.items():
        assert c2[k][:4] == c[:4] and np.array_equal(c2[k].params, c.params)
    for k, im in images.items():
        got = i2[k]
        assert (got.id, got.camera_id, got.name) == (im.id, im.camera_id, im.name)
        assert np.array_equal(got.qvec, im.qvec) and np.array_equal(got.tvec, im.tvec) and np.array_equal(got.xys, im.xys)
        assert np.array_equal(got.point3D_ids, im.point3D_ids) and got.point3D_ids.dtype == np.int64 and got.xys.shape == (len(im.xys), 2)
    for k, p in points.items():
        got = p2[k]
        assert np.array_equal(got.xyz, p.xyz) and np.array_equal(got.rgb, p.rgb) and got.error == p.error
        assert np.array_equal(got.image_ids, p.image_ids) and np.array_equal(got.point2D_idxs, p.point2D_idxs)


def test_intrinsics_by_camera_model_and_rotation():
    assert sorted(C.CAMERA_MODELS) == list(range(11)) and [C.CAMERA_MODELS[k][1] for k in range(11)] == [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]
    for name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"):
        K = C.intrinsic_of(C.Camera(1, name, 10, 10, np.array([70.0, 3.0, 4.0, 0.1, 0.2])))
        assert np.array_equal(K, [[70, 0, 3], [0, 70, 4], [0, 0, 1]]) and K.dtype == np.float64
    for name in ("PINHOLE", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV", "THIN_PRISM_FISHEYE"):
        K = C.intrinsic_of(C.Camera(1, name, 10, 10, np.arange(1.0, 13.0)))
        assert np.array_equal(K, [[1, 0, 3], [0, 2, 4], [0, 0, 1]])
    q = np.array([0.5, 0.5, -0.5, 0.5])
    R = C.qvec2rotmat(q)
    assert np.allclose(R @ R.T, np.eye(3)) and np.isclose(np.linalg.det(R), 1) and np.array_equal(C.qvec2rotmat([1, 0, 0, 0]), np.eye(3))


@pytest.mark.parametrize("run", sorted(RUNS))
def test_file_texts_equal_the_reference(dense, run):
    g = golden()
    before = set(os.listdir(os.path.join(dense, "images")))
    out = C.convert(dense, device="cpu", **RUNS[run])
    assert out["names"] == [str(n) for n in g["names"]]
    written = [str(w) for w in g[run + "/written"]]
    for rel in written:
        path = os.path.join(dense, rel)
        assert os.path.exists(path), rel
        if rel.endswith(".txt"):
            assert open(path).read() == str(g[f"{run}/text/{rel}"]), rel
        else:
            assert open(path, "rb").read() == g["file/" + str(g[f"{run}/copy/{rel}"])].tobytes(), rel
    # ours: the second copy of the pair file, where the loader reads it; nothing else
    assert open(os.path.join(dense, "cams", "pair.txt")).read() == str(g[run + "/text/pair.txt"])
    now = {os.path.relpath(os.path.join(d, f), dense) for d, _, fs in os.walk(dense) for f in fs}
    assert now == set(written) | {"cams/pair.txt"} | {k[5:] for k in g if k.startswith("file/")}
    assert before < set(os.listdir(os.path.join(dense, "images")))
    for i, text in enumerate(out["cam_texts"]):
        assert text == str(g[f"{run}/text/cams/%08d_cam.txt" % i])
    # the in-memory form is what the texts say
    lines = out["cam_texts"][2].splitlines()
    assert np.array_equal(np.array(" ".join(lines[1:5]).split(), np.float64).reshape(4, 4), out["extrinsics"][2])
    assert np.array_equal(np.array(" ".join(lines[7:10]).split(), np.float64).reshape(3, 3), out["intrinsics"][2])
    assert out["intrinsics"][0][0, 0] != out["intrinsics"][0][1, 1] and out["intrinsics"][1][0, 0] == out["intrinsics"][1][1, 1]
    assert np.allclose(np.array(lines[11].split(), np.float64), out["depth_ranges"][2], atol=SCORE_ATOL, rtol=0)
    if run == "max_d":
        assert (out["depth_ranges"][:, 2] == 64).all()
        lo, step, num, hi = out["depth_ranges"].T
        assert np.allclose(step, (hi - lo) / 63 / 2.0, rtol=1e-15)


def test_host_scores_against_the_golden_pair_file(dense):
    g = golden()
    rows = C.read_pair_text(str(g["default/text/pair.txt"]))
    out = C.convert(dense, device="cpu", write=False)
    N = len(rows)
    assert out["score"].shape == (N, N) and out["score"].dtype == np.float64
    assert np.array_equal(out["score"], out["score"].T) and (np.diag(out["score"]) == 0).all()
    for i, row in enumerate(rows):
        assert len(row) == N == len(out["view_sel"][i])                  # six images: the top 10 is the whole row
        for (k, s), (k2, s2) in zip(row, out["view_sel"][i]):
            assert k == k2 and abs(s - s2) <= SCORE_ATOL, (i, k, k2, s, s2)
            assert abs(out["score"][i, k] - s) <= SCORE_ATOL
        assert [k for k, _ in out["view_sel"][i]] == list(np.argsort(out["score"][i])[::-1][:10])
    assert not os.path.exists(os.path.join(dense, "cams"))               # write=False wrote nothing


def test_score_host_form_rules():
    """multiplicity follows image i's list; -1 and out-of-range entries are no points; score[j][i] is a copy; theta0's two sides"""
    points = np.array([[0.0, 0.0, 0.0], [0.0, 10.0, 0.0], [5.0, 0.0, 0.0]])
    centres = np.array([[-10.0, 100.0, 0.0], [10.0, 100.0, 0.0], [0.0, -50.0, 0.0]])
    lists = [np.array([0, -1, 1, 0, 7]), np.array([1, 1, 0]), np.array([-1, 2])]
    offsets = np.cumsum([0] + [len(x) for x in lists])
    obs = np.concatenate(lists).astype(np.int32)
    t = lambda i, j: C.pair_terms_host(i, j, offsets, obs, points, centres, 5.0, 1.0, 10.0)  # noqa: E731
    assert len(t(0, 1)) == 3 and len(t(1, 0)) == 3 and len(t(0, 2)) == 0 and len(t(1, 2)) == 0
    assert t(0, 1)[0] == t(0, 1)[2] != t(0, 1)[1]                        # point 0 twice, in file order
    score = C.pair_scores_host(offsets, obs, points, centres)
    assert score[0, 1] == score[1, 0] == (t(0, 1)[0] + t(0, 1)[1]) + t(0, 1)[2] and score[0, 2] == 0 == score[2, 2]
    theta = np.degrees(np.arccos(np.dot(centres[0] - points[0], centres[1] - points[0]) / np.linalg.norm(centres[0]) / np.linalg.norm(centres[1])))
    assert theta > 5 and np.isclose(t(0, 1)[0], np.exp(-(theta - 5) ** 2 / (2 * 10.0 ** 2)), rtol=1e-14)
    narrow = C.pair_terms_host(0, 1, offsets, obs, points, centres, 30.0, 1.0, 10.0)[0]      # theta below theta0: sigma1
    assert np.isclose(narrow, np.exp(-(theta - 30) ** 2 / 2), rtol=1e-12)


def test_one_line_exits(dense, capsys):
    def last_line(argv):
        with pytest.raises(SystemExit) as e:
            C.main(argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "Traceback" not in err
        return err.strip().splitlines()[-1]

    model = os.path.join(dense, "sparse", "0")
    cameras, images, points = C.read_model(model)
    # image ids that are not 1 .. N
    renumbered = {(k if k != 4 else 9): im._replace(id=(k if k != 4 else 9)) for k, im in images.items()}
    C.write_model(model, cameras, renumbered, points)
    assert "image ids" in last_line(["--dense_folder", dense, "--test"])
    # an image without a valid observation, named
    blind = dict(images)
    blind[2] = images[2]._replace(point3D_ids=np.full(len(images[2].point3D_ids), -1, np.int64))
    C.write_model(model, cameras, blind, points)
    line = last_line(["--dense_folder", dense, "--test"])
    assert "image 2" in line and images[2].name in line
    assert not os.path.exists(os.path.join(dense, "cams"))
    # no model at all
    shutil.rmtree(model)
    assert "cameras.bin" in last_line(["--dense_folder", dense])
    assert "--dense_folder" in last_line([])


def test_parser_has_the_reference_flags():
    p = C.make_parser()
    got = {a.option_strings[0]: (a.default, getattr(a.type, "__name__", None), a.nargs) for a in p._actions if a.option_strings[0] != "-h"}
    assert got == {"--dense_folder": (None, "str", None), "--max_d": (0, "int", None), "--interval_scale": (1, "float", None),
                   "--theta0": (5, "float", None), "--sigma1": (1, "float", None), "--sigma2": (10, "float", None),
                   "--test": (False, None, 0), "--convert_format": (False, None, 0)}
    assert ast.literal_eval(str(golden()["flags"])) == {"default": [], "max_d": ["--max_d", "64", "--interval_scale", "2"]}


def test_convert_format_re_encodes_through_pil(dense):
    from PIL import Image

    C.convert(dense, device="cpu", convert_format=True)
    for name, mode in (("images/00000000.jpg", "RGB"), ("masks/00000000_mask.jpg", "L")):
        with Image.open(os.path.join(dense, name)) as im:
            assert im.format == "JPEG" and im.mode == mode and im.size == (128, 60)
