"""The pair-score kernel of the view selection (csrc/view_select.hip, ufr_view_pair_scores) against its host form
(uforecon_amd.colmap2mvsnet.pair_scores_host), and the converter on the GPU against the golden pair file.

The tolerance is measured, not chosen.  The kernel adds a pair's terms in a tree, the host form (like the reference) in one
running sum in file order, so the two differ by what a reordering of a float64 sum costs, plus a few ulps from the device's
acos and exp.  The yardstick for the first is how far the reference-order sum moves when the same terms are added in REVERSE
order: taken per pair, relative to the pair's score, and the largest such figure over all pairs of ALL the inputs of this file
(CASES) is the yardstick.  A pair's own figure cannot serve: a pair of one or two terms moves by exactly 0 under a reversal, and
one of some dozen terms often does, which says nothing about how the device's acos and exp round -- the lists of length 0, 1
and 63 that the kernel's edges ask for make such pairs.  The kernel may differ from the host form, per pair and relative to
the score, by up to SPREAD_FACTOR = 8 times the yardstick; the factor covers the device's acos and exp differing from numpy's
by a few ulps.  A point whose term is tiny and ill-conditioned (theta near 180 degrees: the exponent is about -150, so an ulp
of theta is 1e-14 of the term) sits in the long lists, where it cannot dominate a score.
The test prints both figures for every input; DESIGN 3.4.7 quotes them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import general_scan_golden as S
from uforecon_amd import _lib, colmap2mvsnet as M, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1
SPREAD_FACTOR = 8.0
PARAMS = (5.0, 1.0, 10.0)          # theta0, sigma1, sigma2: the converter's defaults


def _scene(lengths, seed, special=False):
    """N = len(lengths) images with observation lists of exactly those lengths: -1 entries, repeated indices, image N-1
    sharing nothing with the others (its points come from a pool of its own) when N >= 4, and image 1's list drawn from
    image 0's alone (all of its points shared) when both are long enough."""
    rng = np.random.default_rng(seed)
    N = len(lengths)
    centres = np.stack([650.0 * np.array([np.sin(0.12 * k), -np.cos(0.12 * k), 0.25 + 0.02 * k]) for k in range(N)]) + rng.uniform(-15, 15, (N, 3))
    points = rng.uniform(-120, 120, (420, 3))
    n_special = 0
    if special:                    # for the pair (0, 1): theta near 0 (a point far away), theta near 180 (between the centres)
        mid = 0.5 * (centres[0] + centres[1])
        extra = np.stack([mid + 1e7 * np.array([0.3, 1.0, 0.2]), mid + np.array([1e-3, 2e-3, -1e-3]), 0.25 * centres[0] + 0.75 * centres[1]])
        points = np.concatenate([points, extra])
        n_special = len(extra)
    shared, own = np.arange(0, 300), np.arange(300, 420)
    lists = []
    for k, n in enumerate(lengths):
        pool = own if (N >= 4 and k == N - 1) else shared
        if k == 1 and n > 1 and lengths[0] > 1:
            pool = np.unique(lists[0][lists[0] >= 0])
        li = rng.choice(pool, n, replace=n > len(pool)) if n else np.zeros(0, np.int64)
        if n >= 8:
            li[rng.integers(0, n, max(1, n // 16))] = -1           # no 3-D point
            li[rng.integers(0, n, 3)] = li[0] if li[0] >= 0 else li[1]      # one index several times
        if special and k < 2 and n >= 8:
            li[2:2 + n_special] = np.arange(len(points) - n_special, len(points))
        lists.append(li.astype(np.int32))
    offsets = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    return offsets, np.concatenate(lists).astype(np.int32), points, centres


def _figures(offsets, obs, points, centres, params, got):
    """(the largest reversal spread of the input's pairs, the kernel's largest relative difference from the host form); ``got``
    None: the spread alone"""
    N = len(offsets) - 1
    want = M.pair_scores_host(offsets, obs, points, centres, *params)
    spread = worst = 0.0
    for i in range(N):
        for j in range(i + 1, N):
            terms = M.pair_terms_host(i, j, offsets, obs, points, centres, *params)
            if len(terms) == 0:
                assert want[i, j] == 0.0 and (got is None or got[i, j] == 0.0)
                continue
            fwd, rev = np.add.accumulate(terms)[-1], np.add.accumulate(terms[::-1])[-1]
            assert fwd == want[i, j] > 0
            spread = max(spread, abs(fwd - rev) / fwd)
            if got is not None:
                worst = max(worst, abs(got[i, j] - fwd) / fwd)
    return spread, worst


CASES = {
    "n2": ((257, 65), False), "n2_special": ((257, 257), True), "n3_short": ((0, 1, 64), False), "n3": ((257, 1, 63), False),
    "n4": ((63, 64, 65, 257), False), "n5": ((257, 257, 1, 0, 63), True), "n5_edges": ((64, 65, 63, 257, 257), False),
}


@functools.lru_cache(maxsize=None)
def _case(case):
    lengths, special = CASES[case]
    return _scene(lengths, sorted(CASES).index(case), special)


@functools.lru_cache(maxsize=None)
def yardstick():
    """the largest reversal spread over every pair of every input of CASES: host arithmetic only, computed once"""
    return max(_figures(*_case(case), PARAMS, None)[0] for case in CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_scores_equal_the_host_form_within_the_measured_spread(case):
    lengths = CASES[case][0]
    offsets, obs, points, centres = _case(case)
    assert list(np.diff(offsets)) == list(lengths) and (obs == -1).any() == (max(lengths) >= 8)
    runs = [ops.view_pair_scores(offsets, obs, points, centres, *PARAMS, device=DEV).cpu().numpy() for _ in range(2)]
    got = runs[0]
    N = len(lengths)
    assert got.shape == (N, N) and got.dtype == np.float64
    assert np.array_equal(runs[0], runs[1]), "a rerun gave other bits"
    assert np.array_equal(got, got.T) and (np.diag(got) == 0).all()
    if N >= 4:                                       # the image that shares nothing
        others = [k for k in range(N - 1) if lengths[k] > 1]
        assert (got[N - 1, others] == 0).all() if lengths[N - 1] else True
    spread, worst = _figures(offsets, obs, points, centres, PARAMS, got)
    print(f"{case}: lengths {lengths}: reversal spread {spread:.3e} (yardstick {yardstick():.3e}), kernel against the host form "
          f"{worst:.3e} (bound {SPREAD_FACTOR * yardstick():.3e})")
    assert yardstick() > 0
    assert worst <= SPREAD_FACTOR * yardstick(), (case, worst, yardstick())


def test_theta_equal_to_theta0_and_multiplicity():
    """theta0 set to the angle one shared point gives (the `theta <= theta0` side of the switch: its term is 1 whichever side
    an ulp puts it on); a point twice in image 0 and three times in image 1 counts twice"""
    offsets, obs, points, centres = _scene((257, 257), 11, True)
    p = int(obs[0]) if obs[0] >= 0 else int(obs[1])
    u, v = centres[0] - points[p], centres[1] - points[p]
    theta = float((180 / np.pi) * np.arccos(np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v)))
    params = (theta, 1.0, 10.0)
    got = ops.view_pair_scores(offsets, obs, points, centres, *params, device=DEV).cpu().numpy()
    spread, worst = _figures(offsets, obs, points, centres, params, got)
    print(f"theta0 = theta = {theta!r}: reversal spread {spread:.3e}, kernel against the host form {worst:.3e}")
    assert worst <= SPREAD_FACTOR * yardstick()
    pts = np.array([[0.0, 0.0, 0.0], [3.0, 1.0, 2.0]])
    cen = np.array([[-60.0, 600.0, 10.0], [40.0, 610.0, -5.0]])
    lists = [np.array([0, 1, 0], np.int32), np.array([0, 0, 0, 1], np.int32)]
    off = np.array([0, 3, 7], np.int64)
    ob = np.concatenate(lists)
    got = ops.view_pair_scores(off, ob, pts, cen, *PARAMS, device=DEV).cpu().numpy()
    t = M.pair_terms_host(0, 1, off, ob, pts, cen, *PARAMS)
    # (a count, not a precision statement: one more or one fewer copy of the term would be off by all of t[0])
    assert len(t) == 3 and t[0] == t[2] and abs(got[0, 1] - (2 * t[0] + t[1])) < 1e-6 * t[0] and got[1, 0] == got[0, 1]


def test_one_image_and_empty_lists():
    got = ops.view_pair_scores([0, 5], [0, 1, -1, 1, 0], np.zeros((2, 3)), np.ones((1, 3)), device=DEV).cpu().numpy()
    assert got.shape == (1, 1) and got[0, 0] == 0
    got = ops.view_pair_scores([0, 0, 0, 0], [], np.zeros((0, 3)), np.ones((3, 3)), device=DEV).cpu().numpy()
    assert got.shape == (3, 3) and (got == 0).all()


def test_argument_errors_and_the_next_valid_call():
    lib = _lib.load()
    offsets, obs, points, centres = _scene((65, 64, 63), 3)
    N, n_obs, Mp = 3, len(obs), len(points)
    d_obs, d_pts, d_cen = (torch.from_numpy(a).to(DEV) for a in (obs, points, centres))
    score = torch.full((N, N), -1.0, dtype=torch.float64, device=DEV)
    nbytes = lib.ufr_view_pair_scores_workspace_bytes(N, n_obs)
    assert nbytes >= 8 * (N + 1) + 4 * n_obs
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    good = dict(offsets=offsets.ctypes.data_as(i64p), obs=d_obs.data_ptr(), obs_host=obs.ctypes.data_as(i32p), n_obs=n_obs,
                points=d_pts.data_ptr(), M=Mp, centres=d_cen.data_ptr(), N=N, theta0=5.0, sigma1=1.0, sigma2=10.0,
                score=score.data_ptr(), ws=ws.data_ptr(), ws_bytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ufr_view_pair_scores(a["offsets"], a["obs"], a["obs_host"], a["n_obs"], a["points"], a["M"], a["centres"], a["N"],
                                        a["theta0"], a["sigma1"], a["sigma2"], a["score"], a["ws"], a["ws_bytes"], stream)

    back = offsets.copy()
    back[1], back[2] = back[2], back[1]              # non-monotone
    late = offsets + 1                               # does not start at 0
    bad_hi, bad_lo = obs.copy(), obs.copy()
    bad_hi[7], bad_lo[9] = Mp, -2
    refused = [(dict(offsets=None), b"null"), (dict(obs=None), b"null"), (dict(points=None), b"null"), (dict(centres=None), b"null"),
               (dict(score=None), b"null"), (dict(ws=None), b"null"), (dict(N=0), b"N 0"),
               (dict(offsets=back.ctypes.data_as(i64p)), b"monotone"), (dict(offsets=late.ctypes.data_as(i64p)), b"offsets run"),
               (dict(n_obs=n_obs - 1), b"offsets run"),
               (dict(obs_host=bad_hi.ctypes.data_as(i32p)), b"outside"), (dict(obs_host=bad_lo.ctypes.data_as(i32p)), b"outside"),
               (dict(sigma1=0.0), b"sigma"), (dict(sigma2=-1.0), b"sigma"), (dict(sigma1=float("nan")), b"sigma"),
               (dict(ws_bytes=nbytes - 1), b"workspace too small")]
    for kw, word in refused:
        assert call(**kw) == ERR_ARG, kw
        msg = lib.ufr_last_error()
        assert b"ufr_view_pair_scores" in msg and word in msg, (kw, msg)
    assert lib.ufr_view_pair_scores_workspace_bytes(0, 5) == 0 and b"N 0" in lib.ufr_last_error()
    torch.cuda.synchronize()
    assert (score.cpu().numpy() == -1).all()         # a refused call launched nothing
    assert call() == 0
    spread, worst = _figures(offsets, obs, points, centres, PARAMS, score.cpu().numpy())
    assert worst <= SPREAD_FACTOR * yardstick(), (worst, yardstick())
    # without the host copy the caller vouches for the range; an index outside it is "no point", never a read outside `points`
    wild = obs.copy()
    wild[[3, 70]] = [2 ** 31 - 1, -(2 ** 31)]
    tame = np.where((wild < 0) | (wild >= Mp), -1, wild).astype(np.int32)
    d_wild = torch.from_numpy(wild).to(DEV)
    assert call(obs=d_wild.data_ptr(), obs_host=None) == 0
    first = score.cpu().numpy().copy()
    assert call(obs=torch.from_numpy(tame).to(DEV).data_ptr(), obs_host=tame.ctypes.data_as(i32p)) == 0
    assert np.array_equal(first, score.cpu().numpy())
    with pytest.raises(ops.UfrError):
        ops.view_pair_scores(offsets, bad_hi, points, centres, device=DEV)
    with pytest.raises(ops.UfrError):
        ops.view_pair_scores(offsets, obs, points, centres, device="cpu")


def test_converter_on_the_gpu_writes_the_golden_pair_file(tmp_path):
    """colmap2mvsnet.convert with the kernel's scores: the reference's pair file to the digit (%f), the same ranking"""
    dense = S.write_colmap_scene(tmp_path)
    g = S.golden("colmap_small")
    out = M.convert(dense, device=DEV)
    host = M.convert(dense, device="cpu", write=False)
    assert open(dense + "/pair.txt").read() == open(dense + "/cams/pair.txt").read() == str(g["default/text/pair.txt"])
    assert [[k for k, _ in row] for row in out["view_sel"]] == [[k for k, _ in row] for row in host["view_sel"]]
    rel = np.abs(out["score"] - host["score"]).max() / host["score"].max()
    print(f"converter: kernel scores against the host form: {rel:.3e} of the largest score")
    for row_g, row in zip(M.read_pair_text(str(g["default/text/pair.txt"])), out["view_sel"]):
        assert all(k == k2 and abs(s - s2) <= 5e-7 for (k, s), (k2, s2) in zip(row_g, row))      # what %f carries
