"""-m "not gpu": the host side of the Tacotron feed -- the feeder against the reference feeder's own recorded batches
(tests/golden/reference_tacotron_feeder.npz), the prefetch thread, the ranks' shares, the packed layout against prepare_batch, the
exported symbols, and what the two *_reshape entries do before a device is looked at."""
import ctypes as C
import os

import numpy as np
import pytest

from tacotron_feed_cases import NAMES, example, feed_hp, golden, golden_hp, same_bits, write_directories, write_golden_directories
from tacotron_grad_cases import SMALL, hparams

MAX_ITERS = 8


def _golden_feeder(tmp_path, **kw):
    from twvk_amd.tacotron_feed import DataFeederTacotron
    g = golden()
    path_dict = write_golden_directories(tmp_path)
    f = DataFeederTacotron(list(path_dict), golden_hp(), int(g["batch_size"]), int(g["batches_per_group"]), "train", random_seed=int(g["seed"]),
                           skip_path_filter=False, path_dict=path_dict, **kw)
    f.data_ratio = dict(zip(f.data_dirs, (float(v) for v in g["data_ratio"])))       # (the stand-in's ratios; the rule itself: test below)
    return f


# ---------------------------------------------------------------- the feeder against the reference's recorded batches
def test_batches_equal_the_reference_feeders_bit_for_bit(tmp_path):
    """four groups, two on each side of initial_phase_step: every array the reference fed -- composition, order inside the batch, the
    max + 1 padding frame -- is what next_batch() gives"""
    g = golden()
    f = _golden_feeder(tmp_path)
    assert dict(f._offset) == {} and f._offset["anything"] == 2                   # offsets start at 2
    n, r = int(g["n_batches"]), int(g["reduction_factor"])
    assert n == int(g["groups"]) * int(g["batches_per_group"]) == 12 and int(g["initial_phase_step"]) == 6 and int(g["dir_counts"].sum()) == 36
    for b in range(n):
        examples = f.next_examples()
        ids = [int(ex["mel"][0, 0]) - 1000 for ex in examples]
        assert ids == [int(v) for v in g["feed_order"][b]], (b, ids, g["feed_order"][b])
        from twvk_amd.tacotron_feed import prepare_batch
        got = prepare_batch(examples, r)
        for k in NAMES:
            want = g["batch%d_%s" % (b, k)]
            assert same_bits(got[k], want), (b, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        longest = max(len(ex["linear"]) for ex in examples)
        t_out = got["mel_targets"].shape[1]
        assert t_out % r == 0 and longest + 1 <= t_out < longest + 1 + r           # always a padding frame
        assert not got["mel_targets"][:, longest:].any() and not got["linear_targets"][:, longest:].any()
    assert f._step == n
    # both sides of initial_phase_step were seen: an even split first, then 9 + 3 of a group's 12; the first two groups read every
    # example once (no wrap-around), the last two come back to examples already fed (both directories wrap around and reshuffle)
    per_dir = lambda rows: np.bincount([int(g["example%d_dir" % int(i)]) for i in np.ravel(rows)], minlength=2).tolist()
    assert per_dir(g["feed_order"][0:3]) == [6, 6] and per_dir(g["feed_order"][3:6]) == [6, 6]
    assert per_dir(g["feed_order"][6:9]) == [9, 3] and per_dir(g["feed_order"][9:12]) == [9, 3]
    early, late = np.ravel(g["feed_order"][:6]), np.ravel(g["feed_order"][6:])
    assert len(set(early.tolist())) == early.size and set(late.tolist()) & set(early.tolist())
    assert f._offset[f.data_dirs[0]] < 20 and f._offset[f.data_dirs[1]] < 16


def test_prepare_batch_shuffles_as_the_reference_does(tmp_path):
    """prepare_batch(examples, r, rng) is _prepare_batch(batch, r, rng, 'train'): the shuffle inside it, from the same generator state"""
    from twvk_amd.tacotron_feed import prepare_batch
    rng = np.random.RandomState(3)
    ex = [example(rng, 3 + i, 2 + i, 4, 5, i % 2) for i in range(5)]
    a, b = list(ex), list(ex)
    np.random.RandomState(11).shuffle(a)
    got = prepare_batch(b, 3, np.random.RandomState(11))
    assert [id(x) for x in a] == [id(x) for x in b] and [id(x) for x in a] != [id(x) for x in ex]
    want = prepare_batch(a, 3)
    assert all(same_bits(got[k], want[k]) for k in NAMES)


def test_prefetch_thread_does_not_change_the_order(tmp_path):
    plain = _golden_feeder(tmp_path / "a")
    ahead = _golden_feeder(tmp_path / "b")
    one = [[int(ex["mel"][0, 0]) for ex in batch] for batch in plain.example_batches(40)]
    two = [[int(ex["mel"][0, 0]) for ex in batch] for batch in ahead.example_batches(40, prefetch=True)]
    assert len(one) == 40 and one == two
    assert plain._step == ahead._step == 40


def test_path_rules_test_set_and_ranks(tmp_path):
    from twvk_amd.tacotron_feed import DataFeederTacotron, get_path_dict
    hp = feed_hp(max_iters=MAX_ITERS, min_iters=2, min_tokens=4, reduction_factor=5, num_mels=3, num_freq=4)
    dirs = write_directories(tmp_path, hp, speakers=2, per_speaker=24, seed=1, frames=(8, 38), tokens=(3, 9))
    every = {d: sorted(os.path.join(d, p) for p in os.listdir(d)) for d in dirs}
    ok = lambda p: (lambda z: 10 <= z["linear"].shape[0] <= 35 and len(z["tokens"]) >= 4)(np.load(p))
    assert all(any(ok(p) for p in v) and not all(ok(p) for p in v) for v in every.values())         # (the filter has something to do)
    # the path filter: min_iters * r <= frames <= max_iters * r - r, tokens >= min_tokens; the train set is all but the last n_test of the
    # shuffled paths, the test set the last n_test of the sorted ones
    train = get_path_dict(dirs, hp, "train", 2, np.random.RandomState(5))
    test = get_path_dict(dirs, hp, "test", 2, np.random.RandomState(5))
    rng = np.random.RandomState(5)
    for d in dirs:
        passing, shuffled = [p for p in every[d] if ok(p)], list(every[d])
        rng.shuffle(shuffled)                                  # (one generator over the directories in order, as the reference's)
        assert test[d] == passing[-2:] and len(passing) > 6
        assert train[d] == [p for p in shuffled if ok(p)][:-2] and sorted(train[d]) != train[d]
    unfiltered = get_path_dict(dirs, hp, "train", 2, np.random.RandomState(5), skip_path_filter=True)
    assert all(len(unfiltered[d]) == 22 for d in dirs)
    # the test feeder's static batch: drawn from the last n_test paths of each directory, the same batch every time
    t = DataFeederTacotron(dirs, hp, 4, 8, "test", random_seed=5)
    assert all(t.path_dict[d] == [p for p in every[d] if ok(p)][-4:] for d in dirs)
    first, second = t.next_examples(), t.next_examples()
    names = lambda b: [(ex["speaker_id"], ex["name"]) for ex in b]
    assert names(first) == names(second) and len(first) == 4 and [ex["speaker_id"] for ex in first] == [0, 1, 0, 1]
    last = {os.path.splitext(os.path.basename(p))[0] for d in dirs for p in t.path_dict[d]}
    assert {ex["name"] for ex in first} <= last
    # ranks read disjoint paths, and together all of them
    shares = [get_path_dict(dirs, hp, "train", 1, np.random.RandomState(5 + r), skip_path_filter=True, rank=r, world=2) for r in range(2)]
    for d in dirs:
        assert not set(shares[0][d]) & set(shares[1][d])
        assert set(every[d][0::2]) >= set(shares[0][d]) and set(every[d][1::2]) >= set(shares[1][d]) and len(shares[0][d]) == len(shares[1][d]) == 11
    f0, f1 = (DataFeederTacotron(dirs, hp, 2, 2, "train", random_seed=5, skip_path_filter=True, rank=r, world=2) for r in range(2))
    seen = [{(ex["speaker_id"], ex["name"]) for _ in range(12) for ex in f.next_examples()} for f in (f0, f1)]
    assert seen[0] and seen[1] and not seen[0] & seen[1]
    # data_ratio / main_data_greedy_factor
    hp2 = feed_hp(main_data_greedy_factor=2, main_data=["speaker_1"], **{k: getattr(hp, k) for k in ("max_iters", "min_iters", "min_tokens", "reduction_factor")})
    f = DataFeederTacotron(dirs, hp2, 2, 2, "train", skip_path_filter=True)
    assert [f.data_ratio[d] for d in dirs] == [0.25, 0.75]


# ---------------------------------------------------------------- the packed layout
@pytest.mark.parametrize("shifts", [(0, 0), (1, 3)])
def test_packed_layout_round_trips_on_the_host(shifts):
    """the numpy restatement of the staging kernel on pack_batch's buffer is prepare_batch; also with the sections at odd words and with
    padded sizes larger than needed"""
    from twvk_amd.tacotron_feed import ROW_DTYPE, pack_batch, prepare_batch, stage_numpy, target_frames
    rng = np.random.RandomState(4)
    M, F, r = 3, 5, 5
    ex = [example(rng, nt, nf, M, F, s, c) for nt, nf, s, c in ((4, 7, 0, 1.0), (1, 1, 1, 0.5), (9, 13, 0, 2.0), (2, 14, 1, 1.0))]
    buf, lay = pack_batch(ex, M, F, mel_shift=shifts[0], linear_shift=shifts[1])
    assert buf.dtype == np.uint32 and buf.size == lay["words"] and lay["table_at"] % 2 == 0
    assert (lay["mel_at"] % 4, lay["linear_at"] % 4) == shifts and ROW_DTYPE.itemsize == 32
    want = prepare_batch(ex, r)
    t_in, t_out = want["inputs"].shape[1], want["mel_targets"].shape[1]
    assert (t_in, t_out) == (9, 15) == (9, target_frames(ex, r))
    got = stage_numpy(buf, lay, t_in, t_out, M, F)
    assert all(same_bits(got[k], want[k]) for k in NAMES)
    wide = stage_numpy(buf, lay, t_in + 2, t_out + 3 * r, M, F)
    assert same_bits(wide["mel_targets"][:, :t_out], want["mel_targets"]) and not wide["mel_targets"][:, t_out:].any()
    assert same_bits(wide["inputs"][:, :t_in], want["inputs"]) and not wide["inputs"][:, t_in:].any()
    for bad in ((t_in - 1, t_out), (t_in, 13)):
        with pytest.raises(ValueError):
            stage_numpy(buf, lay, bad[0], bad[1], M, F)
    # packing into a caller's buffer that held something else
    out = np.full(lay["words"] + 7, 0xFFFFFFFF, np.uint32)
    buf2, lay2 = pack_batch(ex, M, F, out=out, mel_shift=shifts[0], linear_shift=shifts[1])
    assert buf2 is out and lay2 == lay
    assert all(same_bits(stage_numpy(out, lay, t_in, t_out, M, F)[k], want[k]) for k in NAMES)


# ---------------------------------------------------------------- the C surface
NEW_SYMBOLS = ("twv_tacotron_decoder_grad_reshape", "twv_tacotron_cbhg_grad_reshape", "twv_tacotron_batch_stage")


def test_symbols_are_exported_and_declared():
    import subprocess
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header and (" T " + name + "\n") in nm, name
    assert "twv_tacotron_feed_row" in header
    for kernel in ("tf_stage_rows_kernel", "tf_stage_tokens_kernel"):
        assert kernel in nm, "the gfx950 kernel %s must be in the library" % kernel


@pytest.fixture(scope="module")
def model():
    from twvk_amd.tacotron import Tacotron
    return Tacotron(hparams(max_iters=MAX_ITERS, **SMALL), num_speakers=2)


def _error(L):
    return L.twv_last_error().decode()


def test_reshape_refuses_what_create_refuses_and_leaves_the_handle(model):
    """t_in 0 and 1025, steps above max_iters, batch 0, T_out above max_iters * r: the same code and the same words from _create and
    _reshape, and the refused handle keeps its sizes (its workspace size and label).  The LDS bound on t_in is part of the shared
    validation (tg_check_sizes); no model twv_tacotron_create accepts reaches it at t_in <= 1024 -- the two recurrent kernels' carves stay
    under 80 KB at the widest accepted sizes -- so no t_in can be shown to be refused by it."""
    L, h = model._L, model._h
    r = model._hparams.reduction_factor
    gd, ge, gp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.twv_tacotron_decoder_grad_create(h, 3, 19, 8, C.byref(gd)) == 0
    assert L.twv_tacotron_cbhg_grad_create(h, 0, 3, 19, C.byref(ge)) == 0
    assert L.twv_tacotron_cbhg_grad_create(h, 1, 3, 40, C.byref(gp)) == 0
    try:
        kept = (L.twv_tacotron_decoder_grad_workspace_bytes(gd), L.twv_tacotron_decoder_grad_route(gd), L.twv_tacotron_cbhg_grad_workspace_bytes(ge),
                L.twv_tacotron_cbhg_grad_workspace_bytes(gp))
        for sizes in ((3, 0, 8), (3, 1025, 8), (3, 19, MAX_ITERS + 1), (3, 19, 0), (0, 19, 8), (-1, 19, 8)):
            fresh = C.c_void_p()
            rc = L.twv_tacotron_decoder_grad_create(h, *sizes, C.byref(fresh))
            words = _error(L)
            assert rc == 1 and not fresh.value, sizes
            assert L.twv_tacotron_decoder_grad_reshape(gd, *sizes) == rc and _error(L) == words, sizes
        for g, which, bad in ((ge, 0, ((3, 0), (3, 1025), (0, 19), (1 << 20, 17))), (gp, 1, ((3, 0), (3, MAX_ITERS * r + 1), (0, 40)))):
            for sizes in bad:
                fresh = C.c_void_p()
                rc = L.twv_tacotron_cbhg_grad_create(h, which, *sizes, C.byref(fresh))
                words = _error(L)
                assert rc == 1 and not fresh.value, (which, sizes)
                assert L.twv_tacotron_cbhg_grad_reshape(g, *sizes) == rc and _error(L) == words, (which, sizes)
        assert kept == (L.twv_tacotron_decoder_grad_workspace_bytes(gd), L.twv_tacotron_decoder_grad_route(gd), L.twv_tacotron_cbhg_grad_workspace_bytes(ge),
                        L.twv_tacotron_cbhg_grad_workspace_bytes(gp))
        assert L.twv_tacotron_decoder_grad_reshape(None, 3, 19, 8) == 1 and L.twv_tacotron_cbhg_grad_reshape(None, 3, 19) == 1
    finally:
        L.twv_tacotron_decoder_grad_destroy(gd); L.twv_tacotron_cbhg_grad_destroy(ge); L.twv_tacotron_cbhg_grad_destroy(gp)


def test_workspace_bytes_and_label_follow_a_reshape(model):
    """over a grid of sizes, going down and back up: _workspace_bytes and the label of the reshaped handle are a fresh handle's"""
    L, h = model._L, model._h
    r = model._hparams.reduction_factor
    grid = [(3, 19, 8), (1, 1, 1), (33, 1024, 8), (2, 129, 3), (3, 19, 8), (16, 130, 1), (1, 1024, MAX_ITERS)]
    gd, ge, gp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.twv_tacotron_decoder_grad_create(h, 5, 7, 2, C.byref(gd)) == 0
    assert L.twv_tacotron_cbhg_grad_create(h, 0, 5, 7, C.byref(ge)) == 0
    assert L.twv_tacotron_cbhg_grad_create(h, 1, 5, 10, C.byref(gp)) == 0
    seen = set()
    try:
        for N, T, steps in grid:
            fd, fe, fp = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert L.twv_tacotron_decoder_grad_create(h, N, T, steps, C.byref(fd)) == 0 and L.twv_tacotron_decoder_grad_reshape(gd, N, T, steps) == 0
            assert L.twv_tacotron_cbhg_grad_create(h, 0, N, T, C.byref(fe)) == 0 and L.twv_tacotron_cbhg_grad_reshape(ge, N, T) == 0
            assert L.twv_tacotron_cbhg_grad_create(h, 1, N, steps * r, C.byref(fp)) == 0 and L.twv_tacotron_cbhg_grad_reshape(gp, N, steps * r) == 0
            try:
                sizes = (L.twv_tacotron_decoder_grad_workspace_bytes(fd), L.twv_tacotron_cbhg_grad_workspace_bytes(fe), L.twv_tacotron_cbhg_grad_workspace_bytes(fp))
                assert sizes == (L.twv_tacotron_decoder_grad_workspace_bytes(gd), L.twv_tacotron_cbhg_grad_workspace_bytes(ge),
                                 L.twv_tacotron_cbhg_grad_workspace_bytes(gp)), (N, T, steps)
                assert all(s > 0 for s in sizes)
                seen.add(sizes)
                assert L.twv_tacotron_decoder_grad_route(fd) == L.twv_tacotron_decoder_grad_route(gd)
                assert L.twv_tacotron_cbhg_grad_route(fe) == L.twv_tacotron_cbhg_grad_route(ge) and L.twv_tacotron_cbhg_grad_route(fp) == L.twv_tacotron_cbhg_grad_route(gp)
            finally:
                L.twv_tacotron_decoder_grad_destroy(fd); L.twv_tacotron_cbhg_grad_destroy(fe); L.twv_tacotron_cbhg_grad_destroy(fp)
        assert len(seen) == len(set(grid))
    finally:
        L.twv_tacotron_decoder_grad_destroy(gd); L.twv_tacotron_cbhg_grad_destroy(ge); L.twv_tacotron_cbhg_grad_destroy(gp)


def test_a_backward_straight_after_a_reshape_is_refused_before_the_device(model):
    """`forwarded` is cleared: the backward's refusal comes before any pointer is used (the dummy pointers are host memory)"""
    L, h = model._L, model._h
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    gd, ge = C.c_void_p(), C.c_void_p()
    assert L.twv_tacotron_decoder_grad_create(h, 3, 19, 8, C.byref(gd)) == 0 and L.twv_tacotron_cbhg_grad_create(h, 0, 3, 19, C.byref(ge)) == 0
    try:
        assert L.twv_tacotron_decoder_grad_reshape(gd, 2, 9, 4) == 0 and L.twv_tacotron_cbhg_grad_reshape(ge, 2, 9) == 0
        assert L.twv_tacotron_decoder_grad_backward(gd, p, p, p, p, p, p, p, None, p, p, p) == 1 and "no forward has been made" in _error(L)
        assert L.twv_tacotron_encoder_grad_backward(ge, p, p, p, p, p, p, None, p, p, p) == 1 and "no forward has been made" in _error(L)
    finally:
        L.twv_tacotron_decoder_grad_destroy(gd); L.twv_tacotron_cbhg_grad_destroy(ge)


def test_batch_stage_refuses_on_the_host():
    """every refusal of twv_tacotron_batch_stage is decided from the host's table before anything is launched: host pointers suffice"""
    from twvk_amd import _lib
    from twvk_amd.tacotron_feed import ROW_DTYPE, ROW_WORDS, pack_batch
    L = _lib.lib()
    rng = np.random.RandomState(0)
    M, F = 3, 5
    ex = [example(rng, 4, 7, M, F), example(rng, 6, 2, M, F)]
    raw = np.zeros(4096 + 4, np.uint32)
    at = (-raw.ctypes.data // 4) % 4                           # a 16-byte aligned start inside raw
    buf, lay = pack_batch(ex, M, F, out=raw[at:at + 4096])
    table = buf[lay["table_at"]:lay["table_at"] + ROW_WORDS * 2].view(ROW_DTYPE)
    outs = np.zeros(64, np.float32)
    o = C.c_void_p(outs.ctypes.data + (-outs.ctypes.data) % 16)

    def call(t_in, t_out, packed=buf.ctypes.data, words=lay["words"], table_at=lay["table_at"], tab=table, batch=2):
        return L.twv_tacotron_batch_stage(C.c_void_p(packed), tab.ctypes.data_as(C.c_void_p), words, lay["tokens_at"], lay["mel_at"], lay["linear_at"], table_at,
                                          lay["total_tokens"], lay["total_frames"], batch, t_in, t_out, M, F, o, o, o, o, o, o, None)
    assert call(5, 10) == 1 and "6 tokens do not fit t_in = 5" in _error(L)
    assert call(6, 6) == 1 and "7 frames do not fit t_out = 6" in _error(L)
    assert call(0, 10) == 1 and call(6, 0) == 1 and call(6, 10, batch=0) == 1
    assert call(6, 10, packed=buf.ctypes.data + 4) == 1 and "16-byte aligned" in _error(L)
    assert call(6, 10, table_at=lay["table_at"] + 1, words=lay["words"] + 1) == 1 and "even word" in _error(L)
    assert call(6, 10, words=lay["words"] - 1) == 1 and "outside its packed_words" in _error(L)
    bad = table.copy()
    bad["frame_offset"][1] = lay["total_frames"]
    assert call(6, 10, tab=bad) == 1 and "table row 1" in _error(L)
    bad = table.copy()
    bad["token_offset"][0] = -1
    assert call(6, 10, tab=bad) == 1 and "table row 0" in _error(L)
