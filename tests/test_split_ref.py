"""The restatement of the two-hand split (tests/split_ref.py) on quarter images small enough to label by hand: every answer below is written out, not computed.
Then the two properties the GPU tests lean on: a mirrored left frame is the mirror image of the unmirrored one, and the rendered two-hand scene of
tests/test_gpu_split.py is separable -- its split IS the two solo frames."""
import os

import numpy as np
import pytest

import mirror_ref
import split_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
FAR, HI = 4000, 650
N = S.NONE


def _split(cells, **kw):
    """cells: a quarter image of depths, 0 = background; one frame"""
    out = S.split(S.frame_of(np.array(cells), FAR, np.random.default_rng(1))[None], kw.pop("lo", 0), HI, FAR, **kw)
    return out["labels"][0].tolist(), out["info"][0].tolist(), int(out["n_components"][0]), out["frames"][0]


def test_two_by_two():
    lab, info, n, frames = _split([[300, 0], [0, 300]])
    assert lab == [[0, N], [N, 3]] and n == 2
    # equal counts: the smaller label (0) is taken first; it is lower (sum_x 0 * 1 < 1 * 1), so the right hand is cell 3 and the left cell 0
    assert info == [[1, 3, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 0, 0, 0, 0]]
    assert (frames[0][4:, 4:] < FAR).any() and (frames[0][:4] == FAR).all() and (frames[0][:, :4] == FAR).all()
    assert (frames[1][:4, :4] < FAR).any() and (frames[1][4:] == FAR).all() and (frames[1][:, 4:] == FAR).all()
    _, info, _, _ = _split([[300, 0], [0, 300]], flags=S.RIGHT_IS_LOW_X)
    assert info == [[1, 0, 0, 0, 0, 0, 0, 0], [1, 3, 1, 1, 1, 1, 1, 1]]
    lab, info, n, _ = _split([[300, 0], [0, 300]], lo=301)      # nothing in range
    assert lab == [[N, N], [N, N]] and n == 0 and info == [[0, N, 0, 0, 0, 0, 0, 0]] * 2


def test_serpentine_is_one_component_through_every_cell():
    m = S.serpentine(9, 5)
    assert m.astype(int).tolist() == [[1] * 9, [0] * 8 + [1], [1] * 9, [1] + [0] * 8, [1] * 9]
    lab, info, n, _ = _split(m * 300)
    assert n == 1 and all(l == (0 if c else N) for row, mrow in zip(lab, m) for l, c in zip(row, mrow))
    # 29 cells; sum_x = 3 * 36 + 8 + 0, sum_y = 9 * (0 + 2 + 4) + 1 + 3; 2 * 116 = 29 * 8: exactly centred, which is NOT low: the right hand of an egocentric camera
    assert info == [[29, 0, 116, 58, 0, 0, 8, 4], [0, N, 0, 0, 0, 0, 0, 0]]
    _, info, _, _ = _split(m * 300, flags=S.RIGHT_IS_LOW_X)
    assert info == [[0, N, 0, 0, 0, 0, 0, 0], [29, 0, 116, 58, 0, 0, 8, 4]]
    big = S.labels_of(np.where(S.serpentine(160, 120), 300, FAR), 0, HI, 65535)
    assert set(np.unique(big)) == {0, N} and (big == 0).sum() == 60 * 160 + 59
    sp = S.spiral(160, 120)
    big = S.labels_of(np.where(sp, 300, FAR), 0, HI, 65535)
    assert set(np.unique(big)) == {0, N} and (big == 0).sum() == sp.sum() > 9000      # one path, every second ring of the image


def test_equal_counts_go_to_the_smaller_label():
    lab, info, n, _ = _split([[300, 300, 0, 0, 310, 310], [0] * 6])
    assert lab == [[0, 0, N, N, 4, 4], [N] * 6] and n == 2
    assert info == [[2, 4, 9, 0, 4, 0, 5, 0], [2, 0, 1, 0, 0, 0, 1, 0]]
    # three of equal count: labels 0 and 2 are taken, 4 is not; 0 is lower than 2
    lab, info, n, _ = _split([[300, 0, 300, 0, 300, 0], [0] * 6])
    assert n == 3 and info == [[1, 2, 2, 0, 2, 0, 2, 0], [1, 0, 0, 0, 0, 0, 0, 0]]
    # the same mean x (1 * 2 == 1 * 2): the smaller label is the lower one
    lab, info, n, _ = _split([[300, 300], [0, 0], [300, 300]])
    assert lab == [[0, 0], [N, N], [4, 4]] and info == [[2, 4, 1, 4, 0, 2, 1, 2], [2, 0, 1, 0, 0, 0, 1, 0]]
    # a larger count wins whatever the labels
    _, info, n, _ = _split([[300, 0, 300, 300, 0, 300, 300, 300], [0] * 8])
    assert n == 3 and info == [[3, 5, 18, 0, 5, 0, 7, 0], [2, 2, 5, 0, 2, 0, 3, 0]]


def test_comb_whose_teeth_join_only_through_max_step():
    comb = [[300, 300, 300, 300, 300], [330, 0, 330, 0, 330], [330, 0, 330, 0, 330]]
    lab, info, n, _ = _split(comb)      # the depth test off: one component
    assert lab == [[0] * 5, [0, N, 0, N, 0], [0, N, 0, N, 0]] and n == 1 and info[0] == [11, 0, 22, 9, 0, 0, 4, 2]
    lab, info, n, _ = _split(comb, max_step=30)
    assert lab == [[0] * 5, [0, N, 0, N, 0], [0, N, 0, N, 0]] and n == 1
    lab, info, n, _ = _split(comb, max_step=29)      # the spine and three teeth
    assert lab == [[0] * 5, [5, N, 7, N, 9], [5, N, 7, N, 9]] and n == 4
    assert info == [[5, 0, 10, 0, 0, 0, 4, 0], [2, 5, 0, 3, 0, 1, 0, 2]]      # the spine (mean x 2) against the first tooth (mean x 0)
    lab, _, n, _ = _split(comb, max_step=0)
    assert lab == [[0] * 5, [5, N, 7, N, 9], [5, N, 7, N, 9]] and n == 4


def test_one_blob_on_either_half_and_exactly_centred():
    absent = [0, N, 0, 0, 0, 0, 0, 0]
    for cells, low in (([[300, 300, 0, 0], [0] * 4], True), ([[0, 0, 300, 300], [0] * 4], False), ([[0, 300, 300, 0], [0] * 4], False)):      # 2 * sum_x against 2 * 3: 2, 10, 6
        blob = [2, cells[0].index(300), 2 * cells[0].index(300) + 1, 0, cells[0].index(300), 0, cells[0].index(300) + 1, 0]
        _, info, n, frames = _split(cells)
        assert n == 1 and info == ([absent, blob] if low else [blob, absent])
        assert (frames[0 if low else 1] == FAR).all()
        _, info, n, _ = _split(cells, flags=S.RIGHT_IS_LOW_X)
        assert info == ([blob, absent] if low else [absent, blob])


def test_min_pixels_boundary():
    cells = [[300, 300, 300, 0, 300, 300, 0, 300], [0] * 8]
    assert _split(cells, min_pixels=1)[2] == 3 and _split(cells, min_pixels=2)[2] == 2 and _split(cells, min_pixels=3)[2] == 1 and _split(cells, min_pixels=4)[2] == 0
    _, info, n, _ = _split(cells, min_pixels=3)
    assert info == [[0, N, 0, 0, 0, 0, 0, 0], [3, 0, 3, 0, 0, 0, 2, 0]]      # alone and on the low side
    _, info, n, frames = _split(cells, min_pixels=4)
    assert info == [[0, N, 0, 0, 0, 0, 0, 0]] * 2 and (frames == FAR).all()
    with pytest.raises(AssertionError):
        _split(cells, min_pixels=0)


def test_foreground_is_a_half_open_range_and_a_cell_is_its_blocks_minimum():
    f = np.full((8, 8), FAR, np.uint16)
    f[1, 2] = 649; f[5, 6] = 650; f[6, 1] = 100
    out = S.split(f[None], 100, 650, FAR, max_step=548)
    assert out["labels"][0].tolist() == [[0, N], [2, N]]      # 649 is in, 650 is out, 100 = range_lo is in; 649 - 100 = 549 apart
    assert S.split(f[None], 100, 650, FAR, max_step=549)["labels"][0].tolist() == [[0, N], [0, N]]
    assert S.split(f[None], 101, 650, FAR)["labels"][0].tolist() == [[0, N], [N, N]]
    # equal counts and equal mean x: label 0 is the lower one, so the left hand; a cell's pixels are copied whole
    assert np.array_equal(out["frames"][0, 1][:4, :4], f[:4, :4]) and (out["frames"][0, 1][4:] == FAR).all() and (out["frames"][0, 1][:, 4:] == FAR).all()
    assert np.array_equal(out["frames"][0, 0][4:, :4], f[4:, :4]) and (out["frames"][0, 0][:4] == FAR).all() and (out["frames"][0, 0][:, 4:] == FAR).all()


def test_a_mirrored_left_frame_unmirrored_is_the_unmirrored_split():
    rng = np.random.default_rng(5)
    cells = np.where(rng.random((3, 9, 14)) < 0.55, rng.integers(200, 640, (3, 9, 14)), 0)
    depth = np.stack([S.frame_of(c, FAR, rng) for c in cells])
    cams = rng.standard_normal((3, 12)).astype(np.float32)
    for flags in (0, S.RIGHT_IS_LOW_X):
        a = S.split(depth, 0, HI, FAR, max_step=40, min_pixels=2, flags=flags, cams=cams)
        b = S.split(depth, 0, HI, FAR, max_step=40, min_pixels=2, flags=flags | S.MIRROR_LEFT, cams=cams)
        assert (a["info"][:, :, 0] > 0).all() and a["frames"][:, 1].tobytes() != b["frames"][:, 1].tobytes()
        assert np.array_equal(a["frames"][:, 0], b["frames"][:, 0]) and np.array_equal(mirror_ref.frames(b["frames"][:, 1]), a["frames"][:, 1])
        assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["labels"], b["labels"])
        assert a["cams"][:, 0].tobytes() == cams.tobytes() == a["cams"][:, 1].tobytes() == b["cams"][:, 0].tobytes()
        assert b["cams"][:, 1].tobytes() == mirror_ref.cams(cams, 56).tobytes()


# ---- the rendered two-hand scene of tests/test_gpu_split.py (split_ref.scene_poses) ----------------------------------------------------------------------------
def test_the_rendered_scene_splits_into_its_two_solo_frames():
    from hand_tracking_samples_amd import native
    m = native.Model(os.path.join(HERE, "golden", "model_hand17.htfx"))
    try:
        solos = [[m.render_mesh(p, S.SCENE_CAM, S.SCENE_W, S.SCENE_H, far=4.0)[0] for p in S.scene_poses(k)] for k in S.SCENES]
    finally:
        m.close()
    for solo in solos:
        assert all(s.max() == S.SCENE_FAR and (s < S.SCENE_HI).sum() > 2000 and ((s < S.SCENE_HI) | (s == S.SCENE_FAR)).all() for s in solo)
        assert S.separable(*solo)
        scene = np.minimum(*solo)
        for flags, order in ((0, (0, 1)), (S.RIGHT_IS_LOW_X, (1, 0))):
            out = S.split(scene[None], 0, S.SCENE_HI, S.SCENE_FAR, min_pixels=S.SCENE_MIN_PIXELS, flags=flags)
            assert out["n_components"][0] == 2
            assert out["frames"][0, 0].tobytes() == solo[order[0]].tobytes() and out["frames"][0, 1].tobytes() == solo[order[1]].tobytes()
