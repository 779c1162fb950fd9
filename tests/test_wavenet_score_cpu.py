"""Host-only side of the WaveNet scoring tests: the window plan, the decomposition the design rests on (hop-aligned windows through
the float64 checker give the whole utterance's values), the route and workspace of every table case, the refusals, the exports, and
the eval_vocoder tool's argument and directory rules."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_cases as SC
import train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(*a, **k):
    import twvk_amd  # noqa: F401
    from twvk_amd import score
    return score.plan(*a, **k)


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def _check_plan(lengths, window, rf, hop, slots):
    from twvk_amd import score as S
    p = _plan(lengths, window, rf, hop, slots)
    R = S.halo(rf, hop)
    rows = p.table.reshape(-1, 5)
    live = rows[rows[:, S.UTT] >= 0]
    assert len(live) == p.n_windows and p.table.shape[1:] == (slots, 5) and p.table.shape[0] == -(-p.n_windows // slots)
    assert (rows[len(live):, S.UTT] == -1).all() and (rows[:len(live), S.UTT] >= 0).all()      # idle slots only at the end of the last batch
    for i, T in enumerate(lengths):
        mine = live[live[:, S.UTT] == i]
        kept = np.zeros(T, np.int64)
        for _, start, n, first, last in mine:
            assert start % hop == 0 and n % hop == 0 and rf < n <= window and start >= 0 and start + n <= T
            assert start + rf <= first <= last <= start + n - 1                        # kept positions are positions the window scores
            kept[first:last + 1] += 1
        assert (kept[rf:] == 1).all() and not kept[:rf].any(), (lengths, window, rf, hop, i)
        bound = 1 + -(-(T - window) // (window - R)) if T > window else 1
        assert 1 <= len(mine) <= bound, (T, window, R, len(mine), bound)
        if T > window:
            assert (mine[:, S.LENGTH] == window).all() and mine[-1, S.START] == T - window     # the last one ends at T
    return p


def test_plan_properties_over_a_seeded_sweep():
    from twvk_amd import score as S
    rng = np.random.RandomState(7)
    for _ in range(300):
        hop = int(rng.choice([1, 16, 32, 64, 300]))
        rf = int(rng.randint(2, 5 * hop + 40))
        R = S.halo(rf, hop)
        window = R + hop * int(rng.randint(1, 9))
        slots = int(rng.randint(1, 9))
        lo = rf // hop + 1
        lengths = [hop * int(rng.randint(lo, lo + 40)) for _ in range(rng.randint(1, 7))]
        _check_plan(lengths, window, rf, hop, slots)


def test_plan_of_the_small_cases():
    from twvk_amd import score as S
    p = _check_plan([600, 900, 1500], 900, 42, 300, 2)
    assert p.table.reshape(-1, 5).tolist() == [[0, 0, 600, 42, 599], [1, 0, 900, 42, 899], [2, 0, 900, 42, 899], [2, 600, 900, 900, 1499]]
    p = _check_plan([600, 900, 1800], 900, 42, 300, 2)          # the last window shifted back; an idle slot in the last batch
    assert p.table.shape == (3, 2, 5) and p.table[2, 1, S.UTT] == -1
    assert p.table.reshape(-1, 5)[2:5].tolist() == [[2, 0, 900, 42, 899], [2, 600, 900, 900, 1499], [2, 900, 900, 1500, 1799]]
    assert _plan([], 900, 42, 300, 2).n_windows == 0


def test_plan_refuses_short_and_misaligned_utterances():
    for lengths in ([600, 0], [0], [601], [901]):
        with pytest.raises(ValueError):
            _plan(lengths, 900, 42, 300, 2)
    with pytest.raises(ValueError):
        _plan([300], 900, 300, 300, 2)                            # T == rf: nothing to score
    with pytest.raises(ValueError):
        _plan([900], 901, 42, 300, 2)                             # window not a hop multiple
    with pytest.raises(ValueError):
        _plan([900], 300, 300, 300, 2)                            # window <= rf
    with pytest.raises(ValueError):
        _plan([1200], 600, 599, 300, 2)                           # more than one window needed, window == halo: no stride


# ---- the decomposition, in the float64 checker --------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SC.IDS)
def test_windows_through_the_checker_give_the_whole_utterance(cid):
    """the property the design rests on: for a hop-aligned start the training graph on the crop gives the whole utterance's values (the
    per-layer front slice of the local condition is shift-invariant at hop multiples).  Agreement to 1e-12 in the quantity every
    scoring comparison uses, e = max|difference| / max|nll64| of the utterance.  Measured: 0.0 in every case but thirty-layers, where
    the float64 library convolutions sum 512- and 960-term products in an order that depends on the crop's length: 2.8e-12 absolute
    on values up to 12.07 (e = 2.3e-13); the checker's own conv1d and matmul forms differ by 3.9e-12 on that utterance."""
    from twvk_amd import score as S
    c = SC.case(cid)
    n64, _ = SC.reference(cid)
    worst = 0.0
    for wf in c.windows:
        p = _plan(c.lengths, wf * c.hop, c.rf, c.hop, c.slots)
        got = [np.full(T - c.rf, np.nan) for T in c.lengths]
        for u, start, n, first, last in p.table.reshape(-1, 5):
            if u < 0:
                continue
            q = None if c.quantized is None else c.quantized[u][start:start + n]
            v = SC.ref_nll(c, c.audios[u][start:start + n], c.mels[u][start // c.hop:(start + n) // c.hop], c.gcs[u], q)
            got[u][first - c.rf:last + 1 - c.rf] = v[first - start - c.rf:last + 1 - start - c.rf]
        for g, w in zip(got, n64):
            assert np.isfinite(g).all()
            worst = max(worst, float(np.abs(g - w).max()) / float(np.abs(w).max()))
    print("%s: windowed against whole-utterance float64, e = %.3g" % (cid, worst))
    assert worst <= 1e-12, (cid, worst)


def test_cases_cover_what_they_are_there_for():
    """stated, so that an edited table shows here: windows per utterance, idle slots, T = rf + 1"""
    from twvk_amd import score as S

    def windows(cid, wf=None):
        c = SC.case(cid)
        t = _plan(c.lengths, (wf or c.windows[0]) * c.hop, c.rf, c.hop, c.slots).table
        return [int((t[:, :, S.UTT] == i).sum()) for i in range(len(c.lengths))], int((t[:, :, S.UTT] < 0).sum()), t
    assert windows("small")[:2] == ([1, 1, 2], 0)
    per, idle, t = windows("small-shifted")
    assert per == [1, 1, 3] and idle == 1 and t.reshape(-1, 5)[4, S.START] == 900
    assert SC.case("ow1").lengths[0] == SC.case("ow1").rf + 1 and SC.case("ow1-staged").lengths[0] == SC.case("ow1-staged").rf + 1
    assert windows("one-cycle")[0] == [1, 3] and SC.case("one-cycle").rf == 1055
    assert windows("thirty-layers")[0] == [13] and SC.case("thirty-layers").rf == 3101
    for cid in ("hop64", "hop32"):
        c = SC.case(cid)
        R = S.halo(c.rf, c.hop)
        assert [w * c.hop for w in c.windows] == [R + c.hop, R + 5 * c.hop]
        assert min(windows(cid, c.windows[0])[0]) >= 1 and max(windows(cid, c.windows[0])[0]) > 2
    assert len(set(SC.case("g64-card5").gcs)) >= 3


# ---- route and workspace --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SC.IDS)
def test_case_is_on_the_route_it_is_meant_to_cover(cid):
    c = SC.case(cid)
    for wf in c.windows:
        route, ws = SC.host_route(c, wf)
        assert {k: route[k] for k in c.route} == c.route, (cid, route)
        assert ws == 4 * int(route["carve_floats"])


def test_every_family_of_the_dispatch_is_in_the_table():
    seen = {(c[5]["lc"], c[5]["head"], c[5]["loss"]) for c in SC.CASES}
    assert {("fused", "skinny", "mol<10>"), ("staged", "skinny", "mol<10>"), ("fused", "skinny", "mol<0>"), ("fused", "gemm", "mol<0>"),
            ("fused", "gemm", "softmax"), ("fused", "skinny", "softmax")} <= seen


@pytest.mark.parametrize("cid", SC.IDS)
def test_workspace_is_smaller_than_the_training_step_s(cid):
    """at the same (slots, window): no TH / SG / per-layer X, no gradient buffers"""
    c = SC.case(cid)
    for wf in c.windows:
        _, ws = SC.host_route(c, wf)
        kw = dict(c.kw)
        kw.pop("gc_ids", None)
        _, train_floats, _ = TC.host_route(B=c.slots, Tm=wf, **kw)
        assert ws < 4 * train_floats, (cid, ws, 4 * train_floats)


def test_workspace_depends_on_slots_and_window_only():
    """nothing in the size knows the utterances: the handle is made from (dims, slots, window) alone, and the size is monotone in both"""
    c = SC.case("small")
    _, a = SC.host_route(c, 3, 2)
    assert SC.host_route(c, 3, 2)[1] == a
    assert SC.host_route(c, 4, 2)[1] > a and SC.host_route(c, 3, 3)[1] > a
    # a list of long utterances through the Python layer plans more windows, not a larger workspace
    from twvk_amd.score import WaveNetScorer
    sc = WaveNetScorer(c.model("cpu"), window=900, slots=2)
    assert sc._L.twv_wavenet_score_workspace_bytes(sc._h) == a and sc.width == 900 - c.rf
    assert _plan([300 * 400], 900, c.rf, 300, 2).n_windows == 1 + -(-(300 * 400 - 900) // 600)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _create(net, slots, window):
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.twv_wavenet_score_create(C.byref(net._dims), slots, window, C.byref(h))
    return rc, h, L


def test_create_refusals():
    c = SC.case("small")
    net = c.model("cpu")
    INVALID, UNSUPPORTED = 1, 2
    for window in (901, 0, -300):                                 # not a hop multiple / nothing
        assert _create(net, 2, window)[0] == INVALID
    big = SC.case("one-cycle")                                    # rf 1055: windows of 900 and 300 samples do not exceed it
    assert _create(big.model("cpu"), 2, 900)[0] == INVALID and _create(big.model("cpu"), 2, 300)[0] == INVALID
    assert _create(net, 0, 900)[0] == INVALID
    # slots x window x 256 >= 2^31 on the fused route; the staged route takes it
    assert _create(net, 64, 131100)[0] == UNSUPPORTED             # 64 * 131100 * 256 = 2^31 + 1.0 M
    rc, h, L = _create(net, 64, 130800)
    assert rc == 0
    L.twv_wavenet_score_destroy(h)
    rc, h, L = _create(SC.case("staged").model("cpu"), 64, 131072)
    assert rc == 0 and b"lc=staged" in L.twv_wavenet_score_route(h)
    L.twv_wavenet_score_destroy(h)
    # what twv_wavenet_train_create refuses (the dims are edited behind the Python model, which has refusals of its own)
    from twvk_amd import _lib

    class Edited(object):
        def __init__(self, **over):
            self._dims = _lib.Dims.from_buffer_copy(net._dims)
            for k, v in over.items():
                setattr(self._dims, k, v)
    for over in (dict(out_channels=31), dict(out_channels=99), dict(out_channels=0), dict(scalar_input=0, quantization_channels=600),
                 dict(scalar_input=0, quantization_channels=1), dict(residual_channels=64), dict(dilation_channels=16), dict(lc_channels=40),
                 dict(gc_channels=0), dict(gc_cardinality=0)):
        assert _create(Edited(**over), 2, 900)[0] == UNSUPPORTED, over
    rc, h, L = _create(Edited(out_channels=96), 2, 900)
    assert rc == 0
    L.twv_wavenet_score_destroy(h)


def test_windows_and_reduce_refuse_bad_lengths_before_anything_is_launched():
    """the arguments are checked on the host first: the (fake, never dereferenced) device pointers are not touched"""
    c = SC.case("small")
    rc, h, L = _create(c.model("cpu"), 2, 900)
    assert rc == 0
    fake = C.c_void_p(0x1000)
    try:
        for lens in ([901, 0], [300 * 4, 0], [-300, 0], [0, 450], [30, 0]):
            arr = np.asarray(lens, np.int32)
            assert L.twv_wavenet_score_windows(h, fake, fake, fake, fake, arr.ctypes.data_as(C.c_void_p), fake, fake, None) == 1, lens
            assert b"length" in L.twv_last_error()
        one = SC.case("one-cycle")
        rc, h2, _ = _create(one.model("cpu"), 2, 1800)
        arr = np.asarray([900, 0], np.int32)                      # a hop multiple, but <= rf = 1055
        assert L.twv_wavenet_score_windows(h2, fake, fake, fake, fake, arr.ctypes.data_as(C.c_void_p), fake, fake, None) == 1
        L.twv_wavenet_score_destroy(h2)
        assert L.twv_wavenet_score_windows(h, None, fake, fake, fake, arr.ctypes.data_as(C.c_void_p), fake, fake, None) == 1
        for lo, hi in (([0, 5], [4, 3]), ([0, 0], [859, 0]), ([-1, 0], [3, 0])):
            a, b = np.asarray(lo, np.int32), np.asarray(hi, np.int32)
            assert L.twv_wavenet_score_reduce(fake, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 2, 858, fake, None) == 1
    finally:
        L.twv_wavenet_score_destroy(h)


def test_scorer_raises_value_error_on_the_host():
    """T <= rf and T != frames * hop (assert_ready_for_upsampling, datafeeder_wavenet.py:38), before the device is touched: the model
    lives on the CPU device here, so any device access would fail differently"""
    from twvk_amd.score import WaveNetScorer
    c = SC.case("one-cycle")
    sc = WaveNetScorer(c.model("cpu"), window=1800, slots=2)
    mel = np.zeros((3, 80), np.float32)
    with pytest.raises(ValueError, match="receptive field"):
        sc.score([np.zeros(900, np.float32)], [mel], [0])
    with pytest.raises(ValueError, match="hop size"):
        sc.score([np.zeros(1800, np.float32)], [mel], [0])
    with pytest.raises(ValueError, match="hop size"):
        sc.held_out_loss([np.zeros(3 * 300 + 7, np.float32)], [mel], [0])
    with pytest.raises(ValueError):
        sc.score([np.zeros(1800, np.float32)], [np.zeros((6, 80), np.float32)], [7])     # speaker id outside the table
    with pytest.raises(ValueError):
        WaveNetScorer(c.model("cpu"), window=900, slots=2)
    with pytest.raises(ValueError):
        WaveNetScorer(c.model("cpu"), window=1801, slots=2)
    assert WaveNetScorer(c.model("cpu")).window == 4 * 1200


# ---- exports ----------------------------------------------------------------------------------------------------------------------
def test_exports_are_in_the_header_and_the_binding():
    from twvk_amd import _lib
    names = ["twv_wavenet_score_create", "twv_wavenet_score_destroy", "twv_wavenet_score_workspace_bytes", "twv_wavenet_score_output_width",
             "twv_wavenet_score_route", "twv_wavenet_score_windows", "twv_wavenet_score_reduce"]
    header = open(os.path.join(ROOT, "include", "twv_amd.h")).read()
    L = _lib.lib()
    for n in names:
        assert re.search(r"\b%s\(" % n, header), n
        assert n in _lib.EXPORTS and hasattr(L, n), n
    # every entry cites its reference lines
    block = header[header.index("WaveNet scoring"):header.index("spectrogram -> waveform")]
    for cite in ("model.py:247-312", "mixture.py:27-81", "model.py:79-80", "datafeeder_wavenet.py:38", "model.py:135", "model.py:290"):
        assert cite in block, cite


# ---- eval_vocoder: arguments and directory rules ----------------------------------------------------------------------------------
def test_eval_vocoder_arguments_and_directory_rules(tmp_path):
    import twvk_amd  # noqa: F401
    from twvk_amd import eval_vocoder as E
    ns = E.build_parser().parse_args(["--load_path", "L", "--data_paths", "a,b"])
    assert (ns.load_path, ns.data_paths, ns.ema, ns.window, ns.slots, ns.per_utterance_out) == ("L", "a,b", False, None, 8, None)
    ns = E.build_parser().parse_args(["--load_path", "L", "--data_paths", "a", "--ema", "--window", "6000", "--slots", "4", "--per_utterance_out", "o.txt"])
    assert (ns.ema, ns.window, ns.slots, ns.per_utterance_out) == (True, 6000, 4, "o.txt")
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(["--data_paths", "a"])
    hop = 4
    d0, d1, d2 = tmp_path / "s0", tmp_path / "s1", tmp_path / "empty"
    for d in (d0, d1, d2):
        d.mkdir()
    rng = np.random.RandomState(0)
    np.savez(str(d0 / "b.npz"), audio=rng.rand(4 * hop + 3).astype(np.float32), mel=rng.rand(4, 80).astype(np.float32))   # cut to frames * hop
    np.savez(str(d0 / "a.npz"), audio=rng.rand(2 * hop, 1).astype(np.float32), mel=rng.rand(2, 80).astype(np.float32))    # (T, 1) as the feeder reshapes
    np.savez(str(d1 / "c.npz"), audio=rng.rand(3 * hop).astype(np.float32), mel=rng.rand(3, 80).astype(np.float32), linear=np.zeros(3))
    (d1 / "notes.txt").write_text("not an example")
    ex = E.list_examples([str(d0), str(d1)])
    assert [(s, os.path.basename(p)) for s, p in ex] == [(0, "a.npz"), (0, "b.npz"), (1, "c.npz")]       # the speaker id is the directory index
    with pytest.raises(SystemExit):
        E.list_examples([str(d0), str(d2)])
    audio, mel = E.load_example(str(d0 / "b.npz"), hop)
    assert audio.shape == (16,) and mel.shape == (4, 80) and audio.dtype == np.float32
    assert E.load_example(str(d0 / "a.npz"), hop)[0].shape == (8,)
    np.savez(str(d1 / "short.npz"), audio=np.zeros(5, np.float32), mel=np.zeros((2, 80), np.float32))
    with pytest.raises(ValueError):
        E.load_example(str(d1 / "short.npz"), hop)

    class FakeScorer(object):                                       # evaluate()'s grouping and averaging, without a device
        def score(self, audios, mels, gcs):
            import torch
            return [torch.full((len(a) - 3,), float(g + 1)) for a, g in zip(audios, gcs)]
    log = []
    rows, per_dir, overall = E.evaluate(FakeScorer(), ex, hop, rf=3, log=log.append, group=2)
    assert [(r[0], os.path.basename(r[1]), r[2], r[3]) for r in rows] == [(0, "a.npz", 5, 1.0), (0, "b.npz", 13, 1.0), (1, "c.npz", 9, 2.0)]
    assert per_dir == {0: (1.0, 18), 1: (2.0, 9)} and overall == (pytest.approx(36.0 / 27.0), 27)
    rows, _, overall = E.evaluate(FakeScorer(), ex, hop, rf=8, log=log.append)                           # a.npz has T = 8 <= rf: skipped, and said so
    assert [os.path.basename(r[1]) for r in rows] == ["b.npz", "c.npz"] and any("skipped" in m and "a.npz" in m for m in log)
