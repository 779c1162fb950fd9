"""-m gpu: Griffin-Lim for utterances of unequal lengths in ONE call (twv_griffin_lim_create_ragged, audio.inv_linear_spectrogram_list /
inv_mel_spectrogram_list, Synthesizer.synthesize(griffin_lim="batched")).  Every utterance of every case of
tests/griffin_lim_ragged_cases.py is held to the project's bar, e_gpu <= max(8 x e_f32, 1e-6) of the peak, against the float64 checker
run on that utterance ALONE at its own length.  Each family yields rows (label, utterance, e_gpu, e_f32, bar);
scripts/griffin_lim_parity.py --ragged records the same rows."""
import ctypes as C

import numpy as np
import pytest

import griffin_lim_cases as G
import griffin_lim_ragged_cases as RG

pytestmark = pytest.mark.gpu


def _run_list(hp, specs, us, basis=None):
    """one list call -> [numpy waveform per utterance]; the cases' arrays are read-only and torch wants writable ones"""
    from twvk_amd.audio import inv_linear_spectrogram_list, inv_mel_spectrogram_list
    specs, us = [np.array(s) for s in specs], [np.array(u) for u in us]
    if basis is not None:
        got = inv_mel_spectrogram_list(specs, hp, uniforms=us, mel_basis=basis)
    else:
        got = inv_linear_spectrogram_list(specs, hp, uniforms=us)
    assert len(got) == len(specs) and all(g.dim() == 1 for g in got)
    if len(got) > 1:                                       # views of one packed buffer, one after the other
        assert all(got[i + 1].data_ptr() == got[i].data_ptr() + 4 * got[i].numel() for i in range(len(got) - 1))
    return [g.cpu().numpy() for g in got]


def _rows(label, got, pairs, hop, Ts, log=print):
    rows = []
    for b, (y64, y32) in enumerate(pairs):
        assert got[b].shape == y64.shape == (hop * (Ts[b] - 1),), (label, b, got[b].shape)
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


def case_rows(name, iters, k, order=None, log=print, tag=""):
    """one row of the case table in one call; order: the utterances (indices into the case) that go into the call, in that order"""
    hp, specs, us, pairs, basis = RG.case(name, iters, k)
    (n_fft, win, hop), Ts, _, _, _ = RG.CASES[name]
    order = list(range(len(Ts))) if order is None else list(order)
    got = _run_list(hp, [specs[i] for i in order], [us[i] for i in order], basis)
    return _rows(RG.label(name, iters, k) + tag, got, [pairs[i] for i in order], hop, [Ts[i] for i in order], log)


ALL_ROWS = [(name, iters, k) for name in sorted(RG.CASES) for iters, k in RG.rows_of(name)]


@pytest.mark.parametrize("name,iters,k", ALL_ROWS, ids=["%s-iters%d-k%g" % r for r in ALL_ROWS])
def test_every_utterance_of_every_case_is_inside_its_own_bar(name, iters, k):
    _assert_rows(case_rows(name, iters, k))


def case_g_order_rows(k, log=print):
    n = len(RG.CASES["G"][1])
    rows = case_rows("G", 2, k, order=range(n - 1, -1, -1), log=log, tag=" reversed")
    for i in range(n):
        rows += case_rows("G", 2, k, order=[i], log=log, tag=" utterance %d alone" % i)
    return rows


@pytest.mark.parametrize("k", RG.CASES["G"][3])
def test_chunk_chain_restarts_whatever_the_order_and_alone(k):
    """case G (1, 2, 3 and 1 de-emphasis chunks) reversed, and every utterance in a call of its own: all rows stay inside the bar"""
    _assert_rows(case_g_order_rows(k))


def equal_lengths_rows(log=print):
    """a ragged handle with equal lengths against the uniform handle on the same inputs; -> (rows, bits equal)"""
    from twvk_amd.audio import inv_linear_spectrogram
    geometry = G.BATCH_GEOMETRY
    hp, spec, u, pairs = G.geometry_case(geometry, 3)
    B = spec.shape[0]
    got = _run_list(hp, [spec[b] for b in range(B)], [u[b] for b in range(B)])
    uniform = inv_linear_spectrogram(np.array(spec), hp, uniforms=np.array(u)).cpu().numpy()
    label = "n_fft %d win %d hop %d T %d iters 3 B %d" % (geometry + (B,))
    rows = _rows("ragged, equal lengths " + label, got, pairs, geometry[2], [geometry[3]] * B, log)
    rows += _rows("uniform, same inputs  " + label, list(uniform), pairs, geometry[2], [geometry[3]] * B, log)
    same = all(np.array_equal(got[b], uniform[b]) for b in range(B))
    log("ragged handle at equal lengths vs uniform handle, %s: bits equal: %s" % (label, same))
    return rows, same


def test_equal_lengths_on_a_ragged_handle_match_the_uniform_handle():
    _assert_rows(equal_lengths_rows()[0])


def test_second_call_on_a_ragged_handle_equals_a_fresh_handle():
    """the plans are made by the first call and reused, the table is copied into the workspace again, the workspace holds the first
    call's magnitudes, frames and signal: the second call's output for other spectra is a fresh handle's, bit for bit"""
    import torch
    from twvk_amd import _lib
    from twvk_amd.audio import inv_linear_spectrogram_list, _ptr
    n_fft, win, hop = 128, 101, 25
    Ts, iters = [21, 4, 9], 3
    hp = G.hparams(n_fft, win, hop, iters)
    calls = [[G.inputs(n_fft, T, 1, 60 + 10 * c + i) for i, T in enumerate(Ts)] for c in range(2)]
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create_ragged(n_fft, hop, win, np.asarray(Ts, np.int32).ctypes.data_as(C.c_void_p), len(Ts), C.byref(h)))
    ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device="cuda:0")
    total = L.twv_griffin_lim_total_samples(h)
    assert total == hop * (sum(Ts) - len(Ts))
    outs = []
    for call in calls:
        out = torch.empty(total, dtype=torch.float32, device="cuda:0")
        s = torch.from_numpy(np.concatenate([spec[0] for spec, _ in call])).cuda()
        uu = torch.from_numpy(np.concatenate([u[0] for _, u in call])).cuda()
        _lib.check(L.twv_inv_linear_spectrogram(h, _ptr(s), _ptr(uu), iters, hp.power, hp.ref_level_db, hp.max_abs_value, hp.min_level_db,
                                                hp.preemphasis, _ptr(ws), _ptr(out), None))
        torch.cuda.synchronize()
        outs.append(out)
    L.twv_griffin_lim_destroy(h)
    assert not torch.equal(outs[0], outs[1])
    for call, out in zip(calls, outs):
        fresh = inv_linear_spectrogram_list([np.array(spec[0]) for spec, _ in call], hp, uniforms=[np.array(u[0]) for _, u in call])
        assert torch.equal(out, torch.cat(fresh))


def norm_mode_rows(kw, log=print):
    """a LINEAR spectrogram with a norm_mode other than 1 takes twv_inv_spectrogram on the ragged handle"""
    from twvk_amd.audio import norm_mode
    n_fft, win, hop = 128, 128, 32
    Ts, iters = [20, 4, 11], 3
    hp = G.hparams(n_fft, win, hop, iters, **kw)
    assert norm_mode(hp) != 1
    specs, us, pairs = [], [], []
    for i, T in enumerate(Ts):
        spec, u = G.inputs(n_fft, T, 1, 80 + i)
        specs.append(spec[0]); us.append(u[0])
        pairs.append(G.checkers(spec[0], u[0], hp, iters, key=("ragged norm", tuple(sorted(kw.items())), i)))
    return _rows("ragged linear norm_mode %d T 20,4,11 iters 3" % norm_mode(hp), _run_list(hp, specs, us), pairs, hop, Ts, log)


NORM_MODES = [{"symmetric_mels": False}, {"allow_clipping_in_normalization": False}, {"signal_normalization": False}]


@pytest.mark.parametrize("kw", NORM_MODES, ids=["mode2", "mode3", "mode0"])
def test_inv_spectrogram_on_a_ragged_handle_linear_other_norm_modes(kw):
    _assert_rows(norm_mode_rows(kw))


def single_call_equality(log=print):
    """REPORTED, not asserted: is each utterance of a ragged call bit-equal to today's B = 1 call on it?  (That depends on hipFFT giving
    the same bits for a transform whatever the plan's batch count.)  -> [(label, utterance, equal)]"""
    from twvk_amd.audio import inv_linear_spectrogram
    report = []
    for name in RG.SMALL:
        if name == RG.MEL_CASE:
            continue
        for iters, k in RG.rows_of(name):
            hp, specs, us, _, _ = RG.case(name, iters, k)
            got = _run_list(hp, specs, us)
            for i in range(len(specs)):
                one = inv_linear_spectrogram(np.array(specs[i])[None], hp, uniforms=np.array(us[i])[None])[0].cpu().numpy()
                same = np.array_equal(got[i], one)
                report.append((RG.label(name, iters, k), i, same))
                log("%-46s utterance %2d: bit-equal to its B = 1 call: %s%s"
                    % (RG.label(name, iters, k), i, same, "" if same else "  (max |diff| %.3e)" % np.abs(got[i] - one).max()))
    log("%d of %d ragged utterances bit-equal to their B = 1 calls" % (sum(r[2] for r in report), len(report)))
    return report


def test_report_bit_equality_with_single_calls():
    """prints the answer (profiles/griffin_lim_parity.txt keeps it); only the shapes of the report are asserted"""
    report = single_call_equality()
    assert len(report) == sum(len(RG.CASES[n][1]) * len(RG.rows_of(n)) for n in RG.SMALL if n != RG.MEL_CASE)


def test_synthesize_batched_writes_what_the_list_call_gives(oracle, tmp_path):
    """the set-up of test_tacotron_gpu.test_synthesize_writes_the_reference_outputs with griffin_lim="batched": the same files; each
    wav is wav_to_int16 of inv_linear_spectrogram_list on the same trimmed spectrograms and uniforms; bytes without a path"""
    import io
    import twvk_amd
    from scipy.io import wavfile
    from twvk_amd.synthesizer import Synthesizer
    from twvk_amd.audio import inv_linear_spectrogram_list
    from twvk_amd.e2e import attention_trim_frames
    from twvk_amd.ops import wav_to_int16
    hp = twvk_amd.default_hparams()
    hp.max_iters, hp.griffin_lim_iters = 6, 3
    d = oracle.taco_dims(max_iters=6, num_freq=hp.num_freq)
    syn = Synthesizer()
    syn.load(oracle.taco_random_tensors(d, seed=5), num_speakers=2, hparams=hp)
    toks = [[5, 9, 33, 12, 1], [7, 7, 1]]
    res = syn.synthesize(tokens=toks, base_path=str(tmp_path), speaker_ids=[1, 0], attention_trim=True, seed=11, griffin_lim="batched")
    assert res == [True, True]
    wavs = sorted(str(p) for p in tmp_path.glob("*.wav")); mels = sorted(str(p) for p in tmp_path.glob("*.npy"))
    assert len(wavs) == 2 and [w.replace(".wav", ".npy") for w in wavs] == mels
    out = syn.infer(toks, speaker_ids=[1, 0])
    F = hp.fft_size // 2 + 1
    ns = [attention_trim_frames(out["alignments"][i].cpu().numpy(), len(out["sequences"][i]), hp.reduction_factor) for i in range(2)]
    lins = [out["linear"][i, :ns[i]].cpu().numpy() for i in range(2)]
    us = [np.random.RandomState(11).rand(1, n, F)[0] for n in ns]
    want = inv_linear_spectrogram_list(lins, hp, uniforms=us)
    for i in range(2):
        assert np.array_equal(np.load(mels[i]), out["mel"][i, :ns[i]].cpu().numpy())
        sr, data = wavfile.read(wavs[i])
        assert want[i].shape == (hp.hop_size * (ns[i] - 1),)
        assert sr == hp.sample_rate and np.array_equal(data, wav_to_int16(want[i][None]).cpu().numpy().reshape(-1))
    blob = syn.synthesize(tokens=toks[:1], speaker_ids=[1], seed=11, griffin_lim="batched")[0]
    sr, data = wavfile.read(io.BytesIO(blob))
    assert sr == hp.sample_rate and np.array_equal(data, wavfile.read(wavs[0])[1])
    with pytest.raises(ValueError):
        syn.synthesize(tokens=toks, griffin_lim="padded")
    # reported, not asserted: the default loop's files against the batched ones
    loop = syn.synthesize(tokens=toks[:1], speaker_ids=[1], seed=11)[0]
    print("synthesize: batched bytes equal the per-utterance loop's: %s" % (loop == blob))


def ragged_parity_report(log=print):
    """every row of every family above (what scripts/griffin_lim_parity.py --ragged records) -> (rows, notes)"""
    rows = []
    for name, iters, k in ALL_ROWS:
        rows += case_rows(name, iters, k, log=log)
    for k in RG.CASES["G"][3]:
        rows += case_g_order_rows(k, log)
    eq_rows, same = equal_lengths_rows(log)
    rows += eq_rows
    for kw in NORM_MODES:
        rows += norm_mode_rows(kw, log)
    return rows, single_call_equality(log)
