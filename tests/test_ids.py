"""Ranked id-coverage buffers without a GPU: the C entry point's export and prototype, what
Scene.render_ids refuses before any upload, the CLI's arguments and writer, rtx.id_matte on CPU
tensors, and the oracle's ranking against pixels worked by hand.

The module also holds the oracle of the id buffers, which tests/test_gpu_ids.py imports:
`rank` restates rtx.h's table rule over sample-major arrays -- a Python loop over the samples,
vectorised over the pixels. It is fed by test_resolved.sample_hits, whose `obj` and `mat` are
the two keys of every sample."""
import numpy as np
import pytest
import torch

import rtx
from rtx import _native as N
from rtx import main as cli

SLOTS = 8


# ---------------------------------------------------------------- the oracle
def rank(keys, hit, ranks):
    """(ids, counts, other) of P pixels from their S samples, sample-major: ``keys`` int
    [S, ...] (>= 0 where ``hit``), ``hit`` bool [S, ...]. Per pixel a table of 8 slots, empty at
    the start; a miss does nothing; a hit with key k counts in the slot that holds k, else takes
    the lowest empty slot as (k, 1), else is dropped. Then the filled slots by count descending,
    equal counts by key ascending, empty slots last: ids (-1) and counts (0) int32
    [..., ranks]; other int32 [...] = dropped + the counts of the ranks >= ``ranks``."""
    hit = np.asarray(hit, bool)
    keys = np.asarray(keys, np.int64)
    assert keys.shape == hit.shape and 1 <= ranks <= SLOTS
    S, shape = hit.shape[0], hit.shape[1:]
    P = int(np.prod(shape, dtype=np.int64))
    k, h = keys.reshape(S, P), hit.reshape(S, P)
    assert (k[h] >= 0).all()
    slot_k = np.full((P, SLOTS), -1, np.int64)
    slot_c = np.zeros((P, SLOTS), np.int64)
    dropped = np.zeros(P, np.int64)
    for s in range(S):
        held = (slot_k == k[s][:, None]) & h[s][:, None]
        slot_c += held
        new = h[s] & ~held.any(axis=1)
        empty = slot_k == -1
        place = new & empty.any(axis=1)
        px = np.nonzero(place)[0]
        at = np.argmax(empty[px], axis=1)  # the lowest empty slot
        slot_k[px, at] = k[s][px]
        slot_c[px, at] = 1
        dropped += new & ~place
    order = np.lexsort((slot_k, -slot_c), axis=1)  # by count descending, then by key ascending
    ids = np.take_along_axis(slot_k, order, axis=1)
    counts = np.take_along_axis(slot_c, order, axis=1)
    assert ((counts == 0) == (ids == -1)).all()
    other = dropped + counts[:, ranks:].sum(axis=1)
    return (ids[:, :ranks].astype(np.int32).reshape(shape + (ranks,)),
            counts[:, :ranks].astype(np.int32).reshape(shape + (ranks,)), other.astype(np.int32).reshape(shape))


def distinct_keys(keys, hit):
    """The number of distinct keys among each pixel's hit samples, int [...]."""
    k = np.where(hit, keys, -1)
    srt = np.sort(k, axis=0)
    return (srt[0] >= 0).astype(np.int64) + ((srt[1:] != srt[:-1]) & (srt[1:] >= 0)).sum(axis=0)


def histogram(keys, hit, n_keys):
    """The full id histogram of each pixel, int [..., n_keys]."""
    k = np.where(hit, keys, n_keys)
    return np.stack([(k == i).sum(axis=0) for i in range(n_keys)], axis=-1)


# ---------------------------------------------------------------- tests
def test_entry_point_is_exported_and_the_abi_is_unchanged():
    lib = N.load()
    assert lib.rtx_abi_version() == 6 and N.ABI_VERSION == 6
    assert "rtx_render_ids" in N.EXPORTS and hasattr(lib, "rtx_render_ids")
    assert len(lib.rtx_render_ids.argtypes) == 10
    assert lib.rtx_render_ids.restype is N.C.c_int
    assert (N.RTX_ID_SLOTS, N.RTX_ID_OBJECT, N.RTX_ID_MATERIAL) == (8, 0, 1)
    assert rtx.ID_NAMES == ("ids", "counts", "other")
    assert "ID_NAMES" in rtx.__all__ and "id_matte" in rtx.__all__
    assert isinstance(rtx.Scene.samples_per_pixel, property)
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    assert sc.samples_per_pixel == 17 == sc.samples * sc.vc.dof_samples * len(sc.vc.motion_times)


def test_header_states_the_prototype():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx.h")).read()
    assert "#define RTX_ID_SLOTS 8" in hdr
    assert "typedef enum rtx_id_key { RTX_ID_OBJECT = 0, RTX_ID_MATERIAL = 1 } rtx_id_key;" in hdr
    flat = " ".join(hdr.split())
    assert ("int rtx_render_ids(rtx_scene* scene, int32_t row0, int32_t nrows, int32_t frame, int32_t key, int32_t ranks, "
            "int32_t* ids_dev, int32_t* counts_dev, int32_t* other_dev, void* hip_stream);") in flat


def test_entry_point_checks_arguments_without_gpu():
    lib = N.load()
    assert lib.rtx_render_ids(None, 0, 1, 0, 0, 4, None, None, None, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_ids: null scene" in lib.rtx_last_error()
    # (a null scene is refused whatever else is passed)
    assert lib.rtx_render_ids(None, -1, -1, -1, 7, 99, 16, 16, 16, None) == N.RTX_ERR_INVALID
    assert b"rtx_render_ids: null scene" in lib.rtx_last_error()


def test_render_ids_refuses_before_any_upload():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    for bad in (("object",), ("ids", "alpha"), (), [], "id", ("ids", "ids")):
        with pytest.raises(ValueError):
            sc.render_ids(buffers=bad)
    for bad in (0, 9, -1, 4.0, "4", None, True, [4]):
        with pytest.raises(ValueError, match="ranks"):
            sc.render_ids(bad)
    for bad in ("objects", "", 0, None, b"object", ("object",)):
        with pytest.raises(ValueError, match="key"):
            sc.render_ids(key=bad)
    for kw in (dict(frame=1), dict(frame=-1), dict(windows=[0.0, 1.0], frame=2), dict(windows=[0.0, 1.0], frame=-1),
               dict(windows=[]), dict(windows=[[0.0, 1.0], [2.0]]), dict(row0=-1), dict(row0=4, nrows=3),
               dict(nrows=-1), dict(row0=7)):
        with pytest.raises(ValueError):
            sc.render_ids(**kw)
    with pytest.raises(IndexError):  # (strip_columns, as render() raises it)
        sc.render_ids(subimage=2, tasks=2)
    bad_out = (
        dict(ids=torch.zeros((6, 8, 4), dtype=torch.int32)),                 # not on the device
        dict(counts=torch.zeros((6, 8, 4), dtype=torch.int64)),              # and not int32
        dict(ids=torch.zeros((6, 8, 8), dtype=torch.int32)),                 # and not [H, W, ranks]
        dict(other=torch.zeros((6, 8, 4), dtype=torch.int32)),               # and not [H, W]
        dict(counts=np.zeros((6, 8, 4), np.int32)),                          # not a tensor
        dict(alpha=torch.zeros((6, 8), dtype=torch.int32)),                  # an unknown name
    )
    for out in bad_out:
        with pytest.raises(ValueError):
            sc.render_ids(out=out)
    with pytest.raises(ValueError, match="out"):                            # not among the requested buffers
        sc.render_ids(buffers=("ids",), out=dict(other=torch.zeros((6, 8), dtype=torch.int32)))
    # good arguments pass every check and the call then fails on its out tensor, still before any upload
    for kw in (dict(ranks=1), dict(ranks=8, key="material"), dict(ranks=np.int64(3), buffers="ids")):
        with pytest.raises(ValueError, match="out"):
            sc.render_ids(out=dict(ids=torch.zeros((1,), dtype=torch.int32)), **kw)
    assert sc._native is None  # nothing was uploaded


def test_cli_ids_arguments(capsys):
    a = cli.parse(["--infile", "s.json", "--ids", "i.npz"])
    assert (a.ids, a.id_ranks, a.id_key, a.outfile) == ("i.npz", None, None, "out.png")
    a = cli.parse(["--infile", "s.json", "--ids", "i.npz", "--id-ranks", "8", "--id-key", "material"])
    assert (a.id_ranks, a.id_key) == (8, "material")
    a = cli.parse(["--infile", "s.json", "--ids", "i.npz", "--resolved", "r.npz", "--aovs", "a.npz", "--subimage", "1",
                   "--tasks", "2", "--id-key", "object", "--id-ranks", "1"])
    assert (a.ids, a.resolved, a.aovs, a.subimage, a.tasks, a.id_key, a.id_ranks) == ("i.npz", "r.npz", "a.npz", 1, 2,
                                                                                     "object", 1)
    a = cli.parse(["--infile", "s.json"])
    assert a.ids is None and a.id_ranks is None and a.id_key is None   # the ordinary render is unchanged
    for bad, word in ((["--ids", "i.npz", "--distributed"], "--distributed"),
                      (["--ids", "i.npz", "--frames", "2"], "--frames"),
                      (["--ids", "i.npz", "--panorama", "8", "4"], "--panorama"),
                      (["--ids", "i.npz", "--id-ranks", "0"], "--id-ranks"),
                      (["--ids", "i.npz", "--id-ranks", "9"], "--id-ranks"),
                      (["--ids", "i.npz", "--id-ranks", "four"], "--id-ranks"),
                      (["--ids", "i.npz", "--id-key", "objects"], "--id-key"),
                      (["--id-ranks", "4"], "--ids"),
                      (["--id-key", "material"], "--ids")):
        with pytest.raises(SystemExit):
            cli.parse(["--infile", "s.json"] + bad)
        assert word in capsys.readouterr().err, bad


def test_cli_writes_the_buffers(tmp_path, monkeypatch):
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(6, 4))
    seen = []

    def fake(ranks, key, buffers, **kw):
        seen.append((ranks, key, tuple(buffers), kw))
        return dict(ids=torch.full((4, 6, ranks), -1, dtype=torch.int32),
                    counts=torch.full((4, 6, ranks), 3, dtype=torch.int32), other=torch.full((4, 6), 2, dtype=torch.int32))
    monkeypatch.setattr(sc, "render_ids", fake)
    path = str(tmp_path / "ids")                                   # (the name is kept as given)
    assert cli.write_ids(sc, cli.parse(["--infile", "s.json", "--ids", path])) == path
    with np.load(path) as z:
        assert sorted(z.files) == ["counts", "ids", "names", "other", "samples"]
        assert z["ids"].dtype == np.int32 and z["ids"].shape == (4, 6, 4) and (z["ids"] == -1).all()
        assert z["counts"].dtype == np.int32 and z["counts"].shape == (4, 6, 4) and (z["counts"] == 3).all()
        assert z["other"].dtype == np.int32 and z["other"].shape == (4, 6) and (z["other"] == 2).all()
        assert z["samples"].shape == () and int(z["samples"]) == 17
        assert z["names"].dtype.kind == "U" and list(z["names"]) == ["plane1", "sphere1", "sphere2"]
    args = cli.parse(["--infile", "s.json", "--ids", str(tmp_path / "m.npz"), "--id-ranks", "2", "--id-key", "material",
                      "--subimage", "1", "--tasks", "3"])
    cli.write_ids(sc, args)
    with np.load(str(tmp_path / "m.npz")) as z:
        assert z["ids"].shape == (4, 6, 2) and list(z["names"]) == ["red", "green", "blue"]
    assert seen == [(4, "object", rtx.ID_NAMES, {}), (2, "material", rtx.ID_NAMES, dict(subimage=1, tasks=3))]


def test_id_matte_by_hand():
    """Two pixels, three ranks, S = 4. Pixel 0: object 5 three times, object 2 once. Pixel 1:
    object 2 twice, one empty rank, and (only here, to show the lookup ignores order) object 7."""
    ids = torch.tensor([[[5, 2, -1], [2, -1, 7]]], dtype=torch.int32)
    counts = torch.tensor([[[3, 1, 0], [2, 0, 1]]], dtype=torch.int32)
    q = np.float32(1.0) / np.float32(4.0)
    m = rtx.id_matte(ids, counts, [2], 4)
    assert m.dtype == torch.float32 and tuple(m.shape) == (1, 2) and m.device == ids.device
    assert np.array_equal(m.numpy(), np.array([[q, 2 * q]], np.float32))
    assert np.array_equal(rtx.id_matte(ids, counts, [5, 2, 2, np.int64(5)], 4).numpy(), np.array([[1.0, 0.5]], np.float32))
    assert np.array_equal(rtx.id_matte(ids, counts, (k for k in (7, 5)), 4).numpy(), np.array([[0.75, 0.25]], np.float32))
    assert not rtx.id_matte(ids, counts, [0, 1, 3], 4).any()                 # an absent object
    third = np.float32(1.0) / np.float32(3.0)                                # one correctly rounded fp32 division
    assert rtx.id_matte(ids, counts, [2], 3).numpy()[0, 0] == third
    for bad in ([], [-1], [0.5], [True], ["sphere"], 3, None):
        with pytest.raises(ValueError):
            rtx.id_matte(ids, counts, bad, 4)
    for bad in (0, -4, 4.0, None, True):
        with pytest.raises(ValueError):
            rtx.id_matte(ids, counts, [2], bad)
    with pytest.raises(ValueError):
        rtx.id_matte(ids, counts[..., :2], [2], 4)
    with pytest.raises(ValueError):
        rtx.id_matte(ids.to(torch.int64), counts, [2], 4)
    with pytest.raises(ValueError):
        rtx.id_matte(ids.numpy(), counts, [2], 4)


def test_scene_id_matte_takes_objects_or_indices():
    sc = rtx.load_bundled_scene("MotionBlur", resolution=(8, 6))
    assert sc.samples_per_pixel == 17
    ids = torch.tensor([[[1, 2, 0, -1]]], dtype=torch.int32)
    counts = torch.tensor([[[9, 5, 3, 0]]], dtype=torch.int32)
    f = np.float32
    assert sc.id_matte(ids, counts, [sc.objects[1], 2]).numpy()[0, 0] == f(14) / f(17)
    assert sc.id_matte(ids, counts, [0, sc.objects[0]]).numpy()[0, 0] == f(3) / f(17)
    assert sc.id_matte(ids, counts, [1], samples=9).numpy()[0, 0] == f(1)
    for bad in ([], [3], [-1], [object()], None):
        with pytest.raises(ValueError):
            sc.id_matte(ids, counts, bad)
    assert sc._native is None


def _pixel(samples):
    """One pixel from a list of keys, None a miss: (keys [S, 1], hit [S, 1])."""
    hit = np.array([[k is not None] for k in samples])
    keys = np.array([[k if k is not None else -1] for k in samples])
    return keys, hit


def test_rank_by_hand():
    # a pixel whose samples all miss
    ids, counts, other = rank(*_pixel([None] * 5), 4)
    assert ids.dtype == counts.dtype == other.dtype == np.int32
    assert ids.shape == counts.shape == (1, 4) and other.shape == (1,)
    assert ids.tolist() == [[-1] * 4] and counts.tolist() == [[0] * 4] and other.tolist() == [0]
    # a tie goes to the smaller key, whichever came first; a miss in between does nothing
    ids, counts, other = rank(*_pixel([7, 3, None, 7, 3, 5]), 4)
    assert ids.tolist() == [[3, 7, 5, -1]] and counts.tolist() == [[2, 2, 1, 0]] and other.tolist() == [0]
    ids, counts, other = rank(*_pixel([3, 7, 7, 3, 5]), 4)
    assert ids.tolist() == [[3, 7, 5, -1]] and counts.tolist() == [[2, 2, 1, 0]]
    # nine distinct keys, the ninth with the most samples: it is dropped, the first eight are kept
    s = [10, 11, 12, 13, 14, 15, 16, 17, 99, 99, 99, 17, 99, 10, 10]
    ids, counts, other = rank(*_pixel(s), 8)
    assert ids.tolist() == [[10, 17, 11, 12, 13, 14, 15, 16]] and counts.tolist() == [[3, 2, 1, 1, 1, 1, 1, 1]]
    assert other.tolist() == [4] and 99 not in ids
    assert counts.sum() + other.sum() == len(s)
    ids, counts, other = rank(*_pixel(s), 1)
    assert ids.tolist() == [[10]] and counts.tolist() == [[3]] and other.tolist() == [12]
    # ranks = 2 over four keys: the tail moves into other
    s = [4, 2, 4, None, 9, 2, 4, 6]
    ids, counts, other = rank(*_pixel(s), 2)
    assert ids.tolist() == [[4, 2]] and counts.tolist() == [[3, 2]] and other.tolist() == [2]
    ids, counts, other = rank(*_pixel(s), 8)
    assert ids.tolist() == [[4, 2, 6, 9, -1, -1, -1, -1]] and counts.tolist() == [[3, 2, 1, 1, 0, 0, 0, 0]]
    assert other.tolist() == [0]
    # key 0 is a key like any other, and a slot once taken is never given up
    ids, counts, other = rank(*_pixel([0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 8, 8]), 8)
    assert ids.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7]] and counts.tolist() == [[2, 1, 1, 1, 1, 1, 1, 1]]
    assert other.tolist() == [3]


def test_rank_is_per_pixel_and_counts_every_hit():
    """Random samples of 6 x 5 pixels over up to 12 keys: every pixel equals its own one-pixel
    ranking, sum(counts) + other is the hit count, and other == 0 gives the full histogram."""
    rs = np.random.RandomState(5)
    keys = rs.randint(0, 12, (24, 6, 5))
    keys[:, :3] = rs.randint(0, 4, (24, 3, 5))  # half the pixels see few keys
    hit = rs.rand(24, 6, 5) < 0.8
    hit[:, 0, 0] = False
    for ranks in (1, 4, 8):
        ids, counts, other = rank(keys, hit, ranks)
        assert ids.shape == counts.shape == (6, 5, ranks) and other.shape == (6, 5)
        assert np.array_equal(counts.sum(axis=-1) + other, hit.sum(axis=0))
        assert ((counts[..., :-1] >= counts[..., 1:]).all()) and ((counts == 0) == (ids == -1)).all()
        for r in range(6):
            for c in range(5):
                one = rank(keys[:, r, c][:, None], hit[:, r, c][:, None], ranks)
                assert np.array_equal(one[0][0], ids[r, c]) and np.array_equal(one[1][0], counts[r, c])
                assert one[2][0] == other[r, c]
    ids, counts, other = rank(keys, hit, 8)
    full = histogram(keys, hit, 12)
    done = other == 0
    assert done[:3].all() and (~done).any() and np.array_equal(distinct_keys(keys, hit) > 8, ~done)
    for i in range(12):
        assert np.array_equal(np.where(ids == i, counts, 0).sum(axis=-1)[done], full[..., i][done])
