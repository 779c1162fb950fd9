"""-m gpu: spectrogram -> waveform (denormalise, Griffin-Lim with librosa's stft/istft conventions, inverse pre-emphasis) on the
device vs the float64 numpy restatement (oracle/audio_np.py).  Floating-point FFT work: tolerance parity, written at each assert."""
import numpy as np
import pytest

import audio_analysis_ref as R
import griffin_lim_cases as G

pytestmark = pytest.mark.gpu


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _ref(lin, u, hp, iters):
    from oracle import audio_np as A
    return np.stack([A.inv_linear_spectrogram(lin[b].T, u[b].T, iters=iters, power=hp.power, ref_level_db=hp.ref_level_db, n_fft=hp.fft_size,
                                              hop=hp.hop_size, win_length=hp.win_size, preemphasis=hp.preemphasis) for b in range(lin.shape[0])])


@pytest.mark.parametrize("iters", [0, 3])
def test_inv_linear_spectrogram_matches_numpy(iters):
    from twvk_amd.audio import inv_linear_spectrogram
    hp = _hp(griffin_lim_iters=iters)
    rng = np.random.RandomState(iters)
    B, T = 2, 14
    lin = rng.uniform(-4.5, 4.5, (B, T, hp.num_freq)).astype(np.float32)       # beyond +-max_abs_value: exercises the clipping
    u = rng.rand(B, T, hp.num_freq).astype(np.float32)
    got = inv_linear_spectrogram(lin, hp, uniforms=u).cpu().numpy()
    want = _ref(lin, u, hp, iters)
    assert got.shape == want.shape == (B, hp.hop_size * (T - 1))
    # tolerance: per utterance, 8 x the distance of the checker's own lines run in float32 (floor 1e-6 of the peak), never above the
    # 2e-4 of the peak this test began with (profiles/griffin_lim_parity.txt: the device sits at 0.8 ... 1.4 x the float32 run here)
    for b in range(B):
        e_gpu, e_f32 = G.rel(got[b], want[b]), G.rel(R.inv_spectrogram_f32(lin[b], u[b], hp, iters), want[b])
        print("iters %d utterance %d: e_gpu %.3e  e_f32 %.3e" % (iters, b, e_gpu, e_f32))
        assert e_gpu <= min(G.bar(e_f32), 2e-4), (b, e_gpu, e_f32)


def test_griffin_lim_sixty_iterations_small_fft():
    """hparams.griffin_lim_iters = 60 on a smaller transform (keeps the float64 restatement fast); the projections do not amplify
    float32 round-off"""
    from twvk_amd.audio import inv_linear_spectrogram
    hp = _hp(griffin_lim_iters=60, fft_size=256, win_size=200, hop_size=50)
    hp.num_freq = 129
    rng = np.random.RandomState(7)
    lin = rng.uniform(-4, 4, (1, 30, 129)).astype(np.float32)
    u = rng.rand(1, 30, 129).astype(np.float32)
    got = inv_linear_spectrogram(lin, hp, uniforms=u).cpu().numpy()
    want = _ref(lin, u, hp, 60)
    e_gpu, e_f32 = G.rel(got[0], want[0]), G.rel(R.inv_spectrogram_f32(lin[0], u[0], hp, 60), want[0])
    print("60 iterations: e_gpu %.3e  e_f32 %.3e" % (e_gpu, e_f32))
    # 8 x the checker's own lines run in float32 through all 60 projections (measured: device 1.0e-6, float32 run 1.4e-6 of the
    # peak), never above the 2e-3 this test began with
    assert e_gpu <= min(G.bar(e_f32), 2e-3), (e_gpu, e_f32)


def test_synthesizer_linear_to_wave_and_save(tmp_path):
    """text -> linear spectrogram (Tacotron) -> wave (Griffin-Lim) -> .wav, the reference synthesizer's own output path"""
    import twvk_amd
    from oracle import oracle as O
    from twvk_amd.tacotron import Synthesizer
    from twvk_amd.audio import inv_linear_spectrogram, save_wav
    hp = _hp(max_iters=4, griffin_lim_iters=2)
    td = O.taco_dims(max_iters=4, num_freq=hp.num_freq)
    syn = Synthesizer(); syn.load(O.taco_random_tensors(td, seed=5), num_speakers=2, hparams=hp)
    out = syn.infer([[5, 9, 33, 12, 1]], speaker_ids=[1])
    wav = inv_linear_spectrogram(out["linear"], hp, seed=3)
    assert wav.shape == (1, hp.hop_size * (4 * hp.reduction_factor - 1)) and np.isfinite(wav.cpu().numpy()).all()
    path = str(tmp_path / "a.wav")
    save_wav(wav[0], path, hp.sample_rate)
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    ref = wav[0].cpu().numpy().copy()
    ref *= 32767 / max(0.01, np.max(np.abs(ref)))                      # utils/audio.py:15 (a quiet signal hits the 0.01 floor)
    assert sr == hp.sample_rate and data.dtype == np.int16 and np.array_equal(data, ref.astype(np.int16))


# ---------------------------------------------------------------------------------------------------------------------------------
# Every geometry, any pre-emphasis, batches, handle reuse and the grid-stride regime at a float32 bar (tests/griffin_lim_cases.py):
# e_gpu <= max(8 x e_f32, 1e-6), e = max|. - float64 checker| / peak per utterance, e_f32 from the checker's lines run in float32.
# Each family below yields rows (label, utterance, e_gpu, e_f32, bar); scripts/griffin_lim_parity.py records the same rows.
def _device(spec, u, hp, inv_basis_of=None):
    from twvk_amd.audio import inv_linear_spectrogram, inv_mel_spectrogram
    spec, u = np.array(spec), np.array(u)              # the cases' arrays are read-only; torch wants writable ones
    if inv_basis_of is not None:
        return inv_mel_spectrogram(spec, hp, uniforms=u, mel_basis=inv_basis_of).cpu().numpy()
    return inv_linear_spectrogram(spec, hp, uniforms=u).cpu().numpy()


def _rows(label, got, pairs, log=print):
    rows = []
    for b, (y64, y32) in enumerate(pairs):
        assert got[b].shape == y64.shape
        e_gpu, e_f32 = G.rel(got[b], y64), G.rel(y32, y64)
        bar = G.bar(e_f32)
        assert bar <= G.OLD_BAR
        rows.append((label, b, e_gpu, e_f32, bar))
        log("%-46s utterance %2d: e_gpu %.3e  e_f32 %.3e  ratio %6.2f  bar %.3e%s"
            % (label, b, e_gpu, e_f32, e_gpu / e_f32 if e_f32 else float("inf"), bar, "" if e_gpu <= bar else "   OUTSIDE"))
    return rows


def _assert_rows(rows):
    bad = [r for r in rows if not r[2] <= r[4]]
    assert not bad, bad


def geometry_rows(geometry, iters, B=3, log=print):
    hp, spec, u, pairs = G.geometry_case(geometry, iters, B=B)
    got = _device(spec, u, hp)
    assert got.shape == (B, geometry[2] * (geometry[3] - 1))
    return _rows("n_fft %d win %d hop %d T %d iters %d B %d" % (geometry + (iters, B)), got, pairs, log)


@pytest.mark.parametrize("iters", [0, 3])
@pytest.mark.parametrize("geometry", G.GEOMETRIES, ids=lambda g: "%d-%d-%d-%d" % g)
def test_griffin_lim_geometries(geometry, iters):
    _assert_rows(geometry_rows(geometry, iters))


@pytest.mark.parametrize("B", [1, 7])
def test_griffin_lim_batches_every_row_another_utterance(B):
    _assert_rows(geometry_rows(G.BATCH_GEOMETRY, 3, B=B))


def _deemphasis_alone(label, geometry, iters, k, B, spec, u, log=print):
    """the de-emphasis kernel by itself: the device's run at k against the float64 recurrence on the device's OWN k = 0 output of the
    same inputs (two k = 0 runs must agree bit for bit for that to mean anything).  Bar: 8 x the distance of the sequential float32
    recurrence on that input, floor 1e-6 of the peak -- the loop's float32 error is not in this comparison."""
    from oracle import audio_np as A
    n_fft, win, hop, T = geometry
    x0 = _device(spec, u, G.hparams(n_fft, win, hop, iters, 0.0))
    assert np.array_equal(x0, _device(spec, u, G.hparams(n_fft, win, hop, iters, 0.0))), "two k = 0 runs of the same inputs differ"
    got = _device(spec, u, G.hparams(n_fft, win, hop, iters, k))
    pairs = [(A.inv_preemphasis(x0[b].astype(np.float64), k), R.inv_preemphasis_f32(x0[b], k)) for b in range(B)]
    return _rows(label + " kernel alone", got, pairs, log)


def deemphasis_rows(k, log=print):
    n_fft, win, hop, T = G.LONG
    spec, u = G.inputs(n_fft, T, 2, G.seed_of(G.LONG, G.LONG_ITERS))
    hp = G.hparams(n_fft, win, hop, G.LONG_ITERS, k)
    pairs = [G.checkers(spec[b], u[b], hp, G.LONG_ITERS, key=(G.LONG, G.LONG_ITERS, 2, k, b)) for b in range(2)]
    got = _device(spec, u, hp)
    assert got.shape == (2, 5950)
    label = "de-emphasis k %g len 5950" % k
    rows = _rows(label, got, pairs, log)
    if k != 0.0:
        rows += _deemphasis_alone(label, G.LONG, G.LONG_ITERS, k, 2, spec, u, log)
    return rows


@pytest.mark.parametrize("k", G.DEEMPH_KS)
def test_deemphasis_any_k_three_chunks(k):
    """a 1024-sample zero-state warm-up, as the kernel had, is 1.5e-3 of the peak away at k = 0.995 and 0.21 at k = 0.999 on these
    inputs (tests/test_griffin_lim_cpu.py shows it on the checker's signal; the library before the fix failed k >= 0.99 here); the
    carried state is exact for every k"""
    _assert_rows(deemphasis_rows(k))


def chunk_edge_rows(geometry, log=print):
    hp, spec, u, pairs = G.geometry_case(geometry, 2, B=1, k=G.EDGE_K)
    got = _device(spec, u, hp)
    label = "chunk edge len %d k %g" % (geometry[2] * (geometry[3] - 1), G.EDGE_K)
    return _rows(label, got, pairs, log) + _deemphasis_alone(label, geometry, 2, G.EDGE_K, 1, spec, u, log)


@pytest.mark.parametrize("geometry", G.EDGES, ids=lambda g: "len%d" % (g[2] * (g[3] - 1)))
def test_deemphasis_chunk_edges(geometry):
    _assert_rows(chunk_edge_rows(geometry))


def test_second_call_on_a_handle_equals_a_fresh_handle():
    """the plans are made by the first call and reused; C2R overwrites spec; the workspace holds the first call's magnitudes, frames and
    signal when the second call starts: its output for other spectra is a fresh handle's, bit for bit"""
    import ctypes as C
    import torch
    from twvk_amd import _lib
    from twvk_amd.audio import inv_linear_spectrogram, _ptr
    n_fft, win, hop, T = G.BATCH_GEOMETRY
    B, iters = 3, 3
    hp = G.hparams(n_fft, win, hop, iters)
    first, second = G.inputs(n_fft, T, B, 41), G.inputs(n_fft, T, B, 42)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create(n_fft, hop, win, T, B, C.byref(h)))
    ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device="cuda:0")
    outs = []
    for spec, u in (first, second):
        out = torch.empty((B, L.twv_griffin_lim_samples(h)), dtype=torch.float32, device="cuda:0")
        s, uu = torch.from_numpy(spec.copy()).cuda(), torch.from_numpy(u.copy()).cuda()
        _lib.check(L.twv_inv_linear_spectrogram(h, _ptr(s), _ptr(uu), iters, hp.power, hp.ref_level_db, hp.max_abs_value, hp.min_level_db,
                                                hp.preemphasis, _ptr(ws), _ptr(out), None))
        torch.cuda.synchronize()
        outs.append(out)
    L.twv_griffin_lim_destroy(h)
    assert not torch.equal(outs[0], outs[1])
    for (spec, u), out in zip((first, second), outs):
        assert torch.equal(out, inv_linear_spectrogram(spec, hp, uniforms=u))


def grid_stride_rows(log=print):
    """B = 17 x T = 1000 at the default geometry, iters = 1: 17.4 M bins and 34.8 M frame samples, both past ga_grid's clamp of 65 535
    blocks x 256, so every GA_STRIDE loop goes round.  Rows cycle through 3 utterances; every row is compared."""
    from scipy.signal import lfilter
    n_fft, win, hop, T = G.STRIDE
    k = 0.97
    spec3, u3 = G.inputs(n_fft, T, G.STRIDE_DISTINCT, G.seed_of(G.STRIDE, 1))
    hp0 = G.hparams(n_fft, win, hop, 1, 0.0)
    pairs3 = []
    for b in range(G.STRIDE_DISTINCT):
        x64 = R.inv_spectrogram(spec3[b], u3[b], hp0, 1)
        pairs3.append((lfilter([1.0], [1.0, -k], x64), R.inv_spectrogram_f32(spec3[b], u3[b], G.hparams(n_fft, win, hop, 1, k), 1)))
    idx = np.arange(G.STRIDE_B) % G.STRIDE_DISTINCT
    assert (G.STRIDE_B * T * (n_fft // 2 + 1)) > 65535 * 256 and G.STRIDE_B * T * n_fft > 65535 * 256
    got = _device(spec3[idx], u3[idx], G.hparams(n_fft, win, hop, 1, k))
    assert got.shape == (G.STRIDE_B, hop * (T - 1))
    return _rows("grid-stride B %d T %d default geometry iters 1" % (G.STRIDE_B, T), got, [pairs3[i] for i in idx], log)


def test_grid_stride_regime():
    _assert_rows(grid_stride_rows())


def inv_mel_rows(case, iters, log=print):
    name, hp, basis = G.mel_cases()[case]
    hp = G.hparams(hp.fft_size, hp.win_size, hp.hop_size, iters, num_mels=hp.num_mels)
    T = {64: 12, 1024: 6}[hp.fft_size]
    spec, u = G.inputs(hp.fft_size, T, 2, 50 + 2 * case + iters, channels=hp.num_mels)
    inv = G.inv_basis_of(basis)
    assert inv.shape == (hp.num_freq, hp.num_mels)
    if case == 1:
        # the clamp of utils/audio.py:190 works: the checker's inv_basis @ amplitudes falls below 1e-10 somewhere
        S = np.power(10.0, (R.denormalize(spec.astype(np.float64), 1, hp.max_abs_value, hp.min_level_db) + hp.ref_level_db) * 0.05)
        lin = S @ inv.astype(np.float64).T
        assert (inv < 0).any() and (lin < 1e-10).any() and (lin > 1e-10).any()
    pairs = [G.checkers(spec[b], u[b], hp, iters, inv, key=("mel", case, iters, b)) for b in range(2)]
    got = _device(spec, u, hp, inv_basis_of=basis)
    return _rows("inv_mel %s n_fft %d iters %d" % (name, hp.fft_size, iters), got, pairs, log)


@pytest.mark.parametrize("iters", [0, 2])
@pytest.mark.parametrize("case", [0, 1], ids=["slaney13x33", "random300x513"])
def test_inv_mel_spectrogram_bases_and_clamp(case, iters):
    """13 x 33: a basis narrower than a wavefront.  300 x 513: both loops of ga_mel_mag_kernel go round (n_mels > 256, nbin > 256)
    and the max(1e-10, .) clamp is hit.  The bar of test_inv_mel_spectrogram_matches_numpy with the float32 loop included."""
    _assert_rows(inv_mel_rows(case, iters))


def parity_report(log=print):
    """every row of every family above (what scripts/griffin_lim_parity.py records)"""
    rows = []
    for geometry in G.GEOMETRIES:
        for iters in (0, 3):
            rows += geometry_rows(geometry, iters, log=log)
    for B in (1, 7):
        rows += geometry_rows(G.BATCH_GEOMETRY, 3, B=B, log=log)
    for k in G.DEEMPH_KS:
        rows += deemphasis_rows(k, log)
    for geometry in G.EDGES:
        rows += chunk_edge_rows(geometry, log)
    for case in (0, 1):
        for iters in (0, 2):
            rows += inv_mel_rows(case, iters, log)
    rows += grid_stride_rows(log)
    return rows
