"""-m gpu: the resampling kernel (twv_resample behind audio.resample) against the float64 numpy checker (tests/resample_ref.py), known
answers no restatement stands behind, the input formats, and wav files of another rate through preprocess.main, audio.load_wav and
generate._load_seed.

Bar of every device-against-checker comparison: max|gpu - f64| <= max(8 x max|f32 checker - f64|, 5e-6 x max|f64|) (resample_ref.bar;
8 and 5e-6 are tests/train_cases.py's RATIO and FLOOR for float32 sums in another order).  The float32 checker is 1.4-2.3e-7 of the
peak from float64 on the first seven pairs' inputs, so the bar is 5e-6 of the peak; one sample of shift or a missing gain s are
0.25-0.46 of it.  resample_ref.PAIRS holds a pair for every route of the kernel (resample_ref.ROUTES: the three instantiations,
chunks 1 and 2, lanes that are not live, a tile above 64 KiB of LDS, rows of 1120 and 1536 taps); on the added pairs the float32
checker is 3e-11 ... 2.9e-7 absolute from float64.  The impulse test needs no bar: one non-zero product per output."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import resample_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_moon_excerpt.npz")
PAIR_IDS = ["%d-%d" % p for p in R.PAIRS]


@functools.lru_cache(maxsize=None)
def _case(pair):
    """five utterances of seeded uniform noise and, computed once, what the checker makes of them: length 1; 50 (all of it inside
    the edge zone); M k (ceil adds nothing); M k + 1 (ceil rounds L / M up); 30 000 (several tiles and a ragged last one)"""
    sr_in, sr_out = pair
    L, M = R.ratio(sr_in, sr_out)
    k = max(2, 3000 // M)
    rng = np.random.RandomState(sr_in // 10 + sr_out)
    wavs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, 50, M * k, M * k + 1, 30000)]
    assert R.out_samples(M * k, sr_in, sr_out) == L * k and R.out_samples(M * k + 1, sr_in, sr_out) == L * k + -(-L // M)
    return wavs, [R.bar(w, sr_in, sr_out) for w in wavs]


@functools.lru_cache(maxsize=None)
def _device_batch(pair):
    from twvk_amd.audio import resample
    out, lengths = resample(_case(pair)[0], pair[0], pair[1])
    return out, lengths


def _route(pair):
    """which kernel the library launches for the pair, from the handle's own accessors"""
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_resample_create(pair[0], pair[1], 30000, 5, C.byref(h)))
    try:
        name, up, taps, rounds = L.twv_resample_kernel_name(h).decode(), L.twv_resample_phases(h), L.twv_resample_taps(h), L.twv_resample_rounds(h)
    finally:
        L.twv_resample_destroy(h)
    lr = int(name[name.index("<") + 1:-1])
    return "%s, L %d, M %d, %d taps, chunks %d (tile of %d outputs), %d lanes of the last wave not live, %d bytes of LDS" % (
        name, up, R.ratio(*pair)[1], taps, rounds // lr, up * rounds, (64 // lr - up % (64 // lr)) % (64 // lr) * lr,
        R.lds_bytes(up, R.ratio(*pair)[1], taps, rounds))


def parity_report(log=print):
    """per pair and utterance: the device's distance to the float64 checker, the float32 checker's, and the bar
    (scripts/resample_parity.py records it)"""
    rows = []
    for pair in R.PAIRS:
        wavs, refs = _case(pair)
        log("%5d -> %5d route: %s" % (pair[0], pair[1], _route(pair)))
        out, lengths = _device_batch(pair)
        got = out.cpu().numpy()
        for b, (w, (y64, bar, d32)) in enumerate(zip(wavs, refs)):
            d, peak = np.abs(got[b, :len(y64)] - y64).max(), np.abs(y64).max()
            rows.append((pair, b, len(w), len(y64), lengths[b], d, d32, bar, peak))
            log("%5d -> %5d utterance %d (%5d -> %5d samples) max|gpu - f64| = %.3e   max|f32 checker - f64| = %.3e   bar = %.3e   peak = %.3f"
                % (pair[0], pair[1], b, len(w), len(y64), d, d32, bar, peak))
    return rows


@pytest.mark.parametrize("pair", R.PAIRS, ids=PAIR_IDS)
def test_parity_ragged_batch(pair):
    wavs, refs = _case(pair)
    out, lengths = _device_batch(pair)
    assert out.shape == (5, R.out_samples(30000, *pair)) and lengths == [len(r[0]) for r in refs]
    got = out.cpu().numpy()
    for b, (y64, bar, d32) in enumerate(refs):
        d = np.abs(got[b, :len(y64)] - y64).max()
        print("%s utterance %d: max|gpu - f64| = %.3e, f32 checker %.3e, bar %.3e" % (pair, b, d, d32, bar))
        assert d <= bar, (pair, b, d, d32, bar)
        assert not got[b, len(y64):].any(), "everything past n_out is exactly 0"


@pytest.mark.parametrize("pair", R.PAIRS, ids=PAIR_IDS)
def test_alone_equals_batch(pair):
    import torch
    from twvk_amd.audio import resample
    wavs, _ = _case(pair)
    out, lengths = _device_batch(pair)
    for b, w in enumerate(wavs):
        one, n = resample(w, pair[0], pair[1])
        assert n == [lengths[b]] and one.shape == (1, lengths[b])
        assert torch.equal(one[0], out[b, :lengths[b]]), (pair, b)


ONE_PER_LR = ((96000, 8000), (96000, 44100), (32000, 11025))          # <64>, <16>, <4> (resample_ref.ROUTES)


@pytest.mark.parametrize("pair", ONE_PER_LR, ids=["%d-%d" % p for p in ONE_PER_LR])
def test_impulse_returns_the_table(pair):
    """x = delta[n - n0]: with t M = q L + p every output is ONE product, 1 * c[p][q + W - n0], plus zeros -- exact in any order, so
    the device must return float32(c[p][k]) of twv_resample_filter_host to the bit (+0 for a tap out of range), no tolerance.  Phase,
    tap index and tile seams at every tile.  n0 = 5000 in 12 000 samples, and n0 on the first tile boundary (rounds * M input samples,
    rounds from twv_resample_rounds), where the impulse's outputs lie in two workgroups."""
    from twvk_amd import _lib
    from twvk_amd.audio import resample
    up, down = R.ratio(*pair)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_resample_create(pair[0], pair[1], 12000, 1, C.byref(h)))
    try:
        taps, rounds = L.twv_resample_taps(h), L.twv_resample_rounds(h)
        tab = np.empty((up, taps), np.float32)
        _lib.check(L.twv_resample_filter_host(h, tab.ctypes.data_as(C.c_void_p)))
    finally:
        L.twv_resample_destroy(h)
    assert (taps, rounds) == (R.ROUTES[pair][2], R.ROUTES[pair][3] * R.ROUTES[pair][4])
    W, tile_out, seam = taps // 2, up * rounds, rounds * down
    for n0, n in ((5000, 12000), (seam, max(12000, seam + 2000))):
        x = np.zeros(n, np.float32)
        x[n0] = 1.0
        out, lengths = resample(x, pair[0], pair[1])
        got = out[0].cpu().numpy()
        t = np.arange(R.out_samples(n, *pair), dtype=np.int64)
        q, p = np.divmod(t * down, up)
        k = q + W - n0
        inside = (k >= 0) & (k < taps)
        want = np.where(inside, tab[p, np.clip(k, 0, taps - 1)], np.float32(0.0))
        assert lengths == [len(t)] and got.shape == want.shape and inside.sum() >= taps * up // down - 1
        if n0 == seam:                                             # outputs of the impulse on either side of the seam
            assert inside[:tile_out].any() and inside[tile_out:].any(), (pair, tile_out)
        assert np.count_nonzero(want) > 0.9 * inside.sum()
        bad = np.flatnonzero(got != want)
        assert not bad.size, (pair, n0, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("pair", [(96000, 8000), (16000, 11025), (96000, 11025)], ids=["96000-8000", "16000-11025", "96000-11025"])
def test_nothing_stale_nothing_behind(pair):
    """the C-ABI itself, one pair per instantiation (<64>; <16> above 64 KiB of LDS; <4>): the workspace holds NaN before the first call
    (the table is uploaded by that call), `out` holds NaN with 1024 marked floats behind it, the batch is (30 000, 1, 0) samples --
    the Python front never passes a length of 0, the host code accepts it (n_out = 0: every tile of the row takes the zero branch) --
    and the input past each length is 7.  Afterwards every row is finite, inside the bar up to n_out, exactly 0 from n_out to the
    stride, and the marks are intact."""
    import torch
    from twvk_amd import _lib
    from twvk_amd.audio import _ptr, _stream
    wavs, refs = _case(pair)
    L = _lib.lib()
    B, n, GUARD, MARK = 3, 30000, 1024, -12345.0
    x = torch.full((B, n), 7.0, device="cuda:0")
    x[0] = torch.from_numpy(wavs[4]).cuda(); x[1, :1] = torch.from_numpy(wavs[0]).cuda()
    lengths = np.asarray([n, 1, 0], np.int32)
    h = C.c_void_p()
    _lib.check(L.twv_resample_create(pair[0], pair[1], n, B, C.byref(h)))
    try:
        stride = int(L.twv_resample_out_samples(h, n))
        n_out = [int(L.twv_resample_out_samples(h, int(v))) for v in lengths]
        assert stride == R.out_samples(n, *pair) and n_out == [stride, len(refs[0][0]), 0]
        ws = torch.full((L.twv_resample_workspace_bytes(h) // 4 + 64,), float("nan"), device="cuda:0")
        buf = torch.full((B * stride + GUARD,), float("nan"), device="cuda:0")
        buf[B * stride:] = MARK
        _lib.check(L.twv_resample(h, _ptr(x), 0, 1, lengths.ctypes.data_as(C.c_void_p), _ptr(ws), _ptr(buf), _stream()))
        torch.cuda.synchronize()
    finally:
        L.twv_resample_destroy(h)
    got = buf.cpu().numpy()
    assert (got[B * stride:] == MARK).all(), "written behind the output"
    got = got[:B * stride].reshape(B, stride)
    assert np.isfinite(got).all(), "a row element was left unwritten"
    for b, (y64, bar, d32) in enumerate((refs[4], refs[0])):
        d = np.abs(got[b, :n_out[b]] - y64).max()
        print("%s utterance %d: max|gpu - f64| = %.3e, f32 checker %.3e, bar %.3e" % (pair, b, d, d32, bar))
        assert d <= bar, (pair, b, d, d32, bar)
        assert not got[b, n_out[b]:].any()
    assert not got[2].any()


def _tone(f, sr, n, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / sr)).astype(np.float32)


def _interior(n_in, sr_in, sr_out):
    """the outputs whose position is more than ceil(64 / s) input samples from either end"""
    L, M = R.ratio(sr_in, sr_out)
    W = R.half_width(sr_in, sr_out)
    t = np.arange(R.out_samples(n_in, sr_in, sr_out))
    pos = t * M / L
    keep = (pos > W) & (pos < n_in - 1 - W)
    assert keep.sum() > 1000
    return t[keep]


def test_zeros_give_zeros():
    from twvk_amd.audio import resample
    out, n = resample(np.zeros(4000, np.float32), 44100, 24000)
    assert n == [2177] and out.shape == (1, 2177) and not out.cpu().numpy().any()


@pytest.mark.parametrize("sr_in,sr_out,f", [(44100, 24000, 1000.0), (44100, 24000, 10000.0), (16000, 24000, 7000.0)],
                         ids=["44100-24000-1k", "44100-24000-10k", "16000-24000-7k"])
def test_pass_band_tone_is_the_same_tone_at_the_new_rate(sr_in, sr_out, f):
    """bar: |float64 checker - analytic| + 5e-6 x 0.5 (on these float32 tones the checker is 1.5e-8, 1.9e-8 and 2.0e-7 from the analytic one)"""
    from twvk_amd.audio import resample
    x = _tone(f, sr_in, 4000)
    t = _interior(4000, sr_in, sr_out)
    want = 0.5 * np.sin(2 * np.pi * f * t / sr_out)
    d_ref = np.abs(R.resample(x, sr_in, sr_out)[t] - want).max()
    out, _ = resample(x, sr_in, sr_out)
    d = np.abs(out[0].cpu().numpy()[t] - want).max()
    print("%d -> %d at %g Hz: max|gpu - analytic| = %.3e, checker %.3e" % (sr_in, sr_out, f, d, d_ref))
    assert d_ref < 1e-6 and d <= d_ref + 5e-6 * 0.5, (d, d_ref)


@pytest.mark.parametrize("sr_in,f", [(44100, 13000.0), (44100, 15000.0), (48000, 14000.0)], ids=["44100-13k", "44100-15k", "48000-14k"])
def test_stop_band_tone_is_gone(sr_in, f):
    """above the new Nyquist frequency nothing may come through (an aliasing kernel leaves up to 0.5); the float64 checker leaves
    2.2e-8, 1.8e-8 and 7.1e-9 of these float32 tones"""
    from twvk_amd.audio import resample
    x = _tone(f, sr_in, 4000)
    t = _interior(4000, sr_in, 24000)
    d_ref = np.abs(R.resample(x, sr_in, 24000)[t]).max()
    out, _ = resample(x, sr_in, 24000)
    d = np.abs(out[0].cpu().numpy()[t]).max()
    print("%d -> 24000 at %g Hz: max|gpu| = %.3e, checker %.3e" % (sr_in, f, d, d_ref))
    assert d_ref < 1e-7 and d < 5e-6 * 0.5, (d, d_ref)


def _fixture():
    z = np.load(GOLDEN)
    return z["frames"], int(z["sample_rate"])


def test_formats_stereo_int16_float_and_device_input():
    import torch
    from twvk_amd.audio import resample
    from twvk_amd._lib import TwvError
    frames, sr = _fixture()
    assert frames.dtype == np.int16 and frames.shape == (6000, 2) and sr == 44100
    mono = (frames / 32768).mean(axis=1)
    y64, bar, d32 = R.bar(mono, sr, 24000)
    assert len(y64) == -((-6000 * 80) // 147) == 3266
    out, n = resample([frames], sr, 24000)                                         # in_format 1, channels 2
    assert n == [3266] and out.shape == (1, 3266)
    d = np.abs(out[0].cpu().numpy() - y64).max()
    print("fixture, stereo int16: max|gpu - f64| = %.3e, f32 checker %.3e, bar %.3e" % (d, d32, bar))
    assert d <= bar
    for label, arg in (("averaged float32", mono.astype(np.float32)), ("stereo float32", (frames / 32768).astype(np.float32)[None]),
                       ("mono int16", None)):
        if arg is None:                                                            # in_format 1, channels 1
            left = np.ascontiguousarray(frames[:, 0])
            want, b2, _ = R.bar(left / 32768, sr, 24000)
            got, _ = resample(left, sr, 24000)
            assert np.abs(got[0].cpu().numpy() - want).max() <= b2, label
            continue
        got, n2 = resample(arg, sr, 24000)
        assert n2 == [3266] and np.abs(got[0].cpu().numpy() - y64).max() <= bar, label
    # (B, len) already on the device, with lengths
    wavs, refs = _case((44100, 24000))
    x = torch.zeros((2, 3000), device="cuda:0")
    x[0] = torch.from_numpy(wavs[4][:3000]).cuda(); x[1, :1717] = torch.from_numpy(wavs[4][:1717]).cuda()
    x[1, 1717:] = 7.0                                                              # past an utterance's length nothing is read
    got, n3 = resample(x, 44100, 24000, lengths=[3000, 1717])
    assert n3 == [1633, 935] and got.shape == (2, 1633) and got.device == x.device
    got = got.cpu().numpy()
    for b, m in enumerate((3000, 1717)):
        want, b3, _ = R.bar(wavs[4][:m], 44100, 24000)
        assert np.abs(got[b, :n3[b]] - want).max() <= b3 and not got[b, n3[b]:].any()
    with pytest.raises(TwvError, match="longer than max_samples_in"):
        resample(x, 44100, 24000, lengths=[3001, 1717])
    with pytest.raises(ValueError):
        resample(np.zeros(10, np.int32), 44100, 24000)


def test_wavs_of_another_rate_through_every_layer(tmp_path):
    """44.1 kHz stereo int16 files (the layout of the reference's own data) -> preprocess.main -> npz examples; audio.load_wav and
    generate._load_seed on the same files"""
    from scipy.io import wavfile
    import twvk_amd
    from twvk_amd import audio, generate, preprocess
    hp = twvk_amd.default_hparams()
    sr = hp.sample_rate
    assert sr == 24000

    def tone(rate, seed):
        t = np.arange(2 * rate) / rate
        env = np.clip(np.sin(np.pi * t / 2.0) * 3, 0, 1)                              # quiet at both ends: the trim has work to do
        return env * (0.4 * np.sin(2 * np.pi * 440 * t) + 0.002 * np.random.RandomState(seed).randn(len(t)))

    src = tmp_path / "wav"
    src.mkdir()
    frames, rate = _fixture()
    for i in range(2):
        x = np.clip(tone(44100, i) * 32767, -32768, 32767).astype(np.int16)
        wavfile.write(str(src / ("a%d.wav" % i)), 44100, np.stack([x, x if i else (x * 0.5).astype(np.int16)], axis=1))
    wavfile.write(str(src / "a2.wav"), rate, frames)
    wavfile.write(str(src / "b0.wav"), sr, np.clip(tone(sr, 1) * 32767, -32768, 32767).astype(np.int16))
    r = preprocess.main(["--in_dir", str(src), "--out_dir", str(tmp_path / "data"), "--batch_size", "3"], log=lambda s: None)
    assert [os.path.basename(p) for p in r["written"]] == ["a0.npz", "a1.npz", "a2.npz", "b0.npz"] and not r["skipped"]
    ex = {os.path.basename(p)[:2]: dict(np.load(p)) for p in r["written"]}
    for d in ex.values():
        T = int(d["mel_frames"])
        assert d["audio"].shape == (T * hp.hop_size,) and d["mel"].shape == (T, hp.num_mels) and d["linear"].shape == (T, hp.num_freq)
        assert np.isfinite(d["mel"]).all() and np.abs(d["audio"]).max() <= 1.0
    # the file already at 24 kHz (a chunk of its own): exactly what the strict reader's path gives
    old = preprocess.process_batch([preprocess.read_wav(str(src / "b0.wav"), sr)], hp)[0]
    for key in ("audio", "mel", "linear", "time_steps", "mel_frames"):
        assert np.array_equal(ex["b0"][key], old[key]), key
    # the same tone resampled from 44.1 kHz: as many frames (one either way) and the same mel bin on top
    T0, T1 = int(ex["b0"]["mel_frames"]), int(ex["a1"]["mel_frames"])
    assert abs(T0 - T1) <= 1 and T0 > 100
    lo, hi = T0 // 4, 3 * T0 // 4
    top = ex["b0"]["mel"][lo:hi].argmax(axis=1)
    assert (top == top[0]).all() and (ex["a1"]["mel"][lo:hi].argmax(axis=1) == top[0]).all()
    assert (ex["a0"]["mel"][lo:hi].argmax(axis=1) == top[0]).all()
    # a chunk that mixes rates: the 24 kHz file by the strict reader, the other by load_wav's kernel
    both = preprocess.read_chunk([str(src / "b0.wav"), str(src / "a2.wav")], sr)
    assert np.array_equal(both[0], preprocess.read_wav(str(src / "b0.wav"), sr))
    y64, bar, _ = R.bar((frames / 32768).mean(axis=1), rate, sr)
    got = audio.load_wav(str(src / "a2.wav"), sr)
    assert got.dtype == np.float32 and got.shape == y64.shape and np.abs(got - y64).max() <= bar
    assert np.array_equal(both[1], got)
    seed = generate._load_seed(str(src / "a2.wav"), sr)
    assert seed.dtype == np.float32 and seed.shape == (-((-6000 * 80) // 147),) and np.array_equal(seed, got)
    with pytest.raises(ValueError, match="resampling is not built"):
        preprocess.read_wav(str(src / "a2.wav"), sr)
