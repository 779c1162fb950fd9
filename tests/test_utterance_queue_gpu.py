"""-m gpu: the utterance queue (WaveNetModel.generate_list, twv_wavenet_reset_streams, twv_wavenet_queue_stage / _collect,
e2e.texts_to_waves) bit for bit against the CPU oracle run ONE UTTERANCE AT A TIME at B = 1 from a fresh state.

Every utterance has its own mel, gc id, seed and uniforms (tests/sensitive_inputs.py: shifted head, every selection on its edge,
conditions asserted on the oracle's output), built once per (model, utterance) and shared by the cases (nobody writes to them).  A
slot that is refilled must give the new utterance the samples of a freshly initialised model, and its neighbours -- on the same
XCD, in the same chain workgroup, in the same launch -- the samples of an uninterrupted run: a reset that misses part of a
stream's state, touches a neighbour's, or clears something the launch shares shows as a sample mismatch.  Hop 300, 1-4 frames per
utterance."""
import ctypes as C

import numpy as np
import pytest

from helpers import first_mismatch, make_case, make_model, sensitive_mol, sensitive_onehot
from sensitive_inputs import shift_mol_head

pytestmark = pytest.mark.gpu

HOP = 300


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dil7(nl):
    return ([1, 2, 4, 8, 16, 32, 64] * 5)[:nl]


_models = {}
_utts = {}


def _mol11(oracle):
    """the 11-layer S = 512 MoL stack of tests/test_xcd_relay_gpu.py (waves of 5, 5 and 1 layers)"""
    if "mol11" not in _models:
        dil = _dil7(11)
        d, tensors, blob = make_case(oracle, dil, shift=5.0)
        _models["mol11"] = (d, tensors, blob, dil)
    return _models["mol11"]


def _utterance(oracle, key, d, blob, uid, frames):
    """utterance `uid` of `frames` frames for model `key`: dict(mel, gc, seed, u, want) -- want is the oracle's B = 1 run from a fresh
    state"""
    k = (key, uid, frames)
    if k not in _utts:
        rng = np.random.RandomState(1000 * uid + frames)
        mel = rng.uniform(-4, 4, (frames, 80)).astype(np.float32)
        gc = np.array([uid % 2], np.int32)
        U = oracle.upsample(d, blob, mel[None])
        if d.scalar_input:
            seed = (2 * rng.rand(1) - 1).astype(np.float32)
            u, want = sensitive_mol(oracle, d, blob, U, gc, seed, 1, frames * HOP, seed=2 + uid)
        else:
            seed = rng.randint(d.Q, size=1).astype(np.int32)
            u, want = sensitive_onehot(oracle, d, blob, U, gc, seed, rng.random_sample((1, frames * HOP)), 1.0)
        _utts[k] = dict(mel=mel, gc=int(gc[0]), seed=seed[0], u=u[0], want=want[0])
    return _utts[k]


def _utterances(oracle, key, d, blob, lengths, first_uid=0):
    return [_utterance(oracle, key, d, blob, first_uid + i, n) for i, n in enumerate(lengths)]


def _run_list(m, utts, **kw):
    got = m.generate_list([x["mel"] for x in utts], [x["gc"] for x in utts], [x["seed"] for x in utts], [x["u"] for x in utts], **kw)
    assert len(got) == len(utts)
    for i, (g, x) in enumerate(zip(got, utts)):
        g = g.cpu().numpy()
        assert g.shape == x["want"].shape and g.dtype == x["want"].dtype, (i, g.shape, g.dtype)
        assert first_mismatch(g, x["want"]) is None, ("utterance", i, first_mismatch(g, x["want"]))
    assert m.status() == 0


CASE1 = [1, 3, 2, 4, 1, 1, 2, 3]


# ---------------------------------------------------------------- 1. wn_xcd_generate_kernel, fused conditioning
@pytest.mark.parametrize("check", [True, False])
@pytest.mark.parametrize("order", ["longest_first", "fifo"])
@pytest.mark.parametrize("chunk_frames", [1, 2])
def test_list_on_the_xcd_kernel(torch_cuda, oracle, chunk_frames, order, check):
    d, tensors, blob, dil = _mol11(oracle)
    m = make_model(3, dil, tensors)
    assert m.kernel_name() == "wn_xcd_generate_kernel" and m.fused_conditioning()
    _run_list(m, _utterances(oracle, "mol11", d, blob, CASE1), chunk_frames=chunk_frames, order=order, check=check)


# ---------------------------------------------------------------- 2. two streams per XCD
CASE2 = [2, 2, 2, 2, 2, 2, 2, 2, 1, 2, 1, 1, 2, 1]


def test_partial_restart_with_two_streams_per_xcd(torch_cuda, oracle):
    """11 slots: XCDs 0-2 carry two chain workgroups each (slots b and b + 8) that share the XCD's skip / conv1 workgroups.  At the
    boundary behind chunk 0 only slots 8 and 10 take a new utterance while their XCD partners 0 and 2 carry on"""
    from twvk_amd import queue as Q
    p = Q.plan(CASE2, 11, 1, "fifo")
    restarts = {s for s in range(11) if p.table[1, s, Q.START]}
    busy = {s for s in range(11) if p.table[1, s, Q.UTT] >= 0}
    assert restarts == {8, 10} and restarts < busy, (restarts, busy)
    for s in restarts:                                                   # the partner on the same XCD continues its utterance
        assert p.table[1, s - 8, Q.UTT] == p.table[0, s - 8, Q.UTT] >= 0 and not p.table[1, s - 8, Q.START]
    d, tensors, blob, dil = _mol11(oracle)
    m = make_model(11, dil, tensors)
    assert m.kernel_name() == "wn_xcd_generate_kernel" and m.fused_conditioning()
    _run_list(m, _utterances(oracle, "mol11", d, blob, CASE2, first_uid=20), chunk_frames=1, order="fifo")


# ---------------------------------------------------------------- 3. wn_xcd_many_kernel
def test_list_on_the_many_streams_kernel(torch_cuda, oracle):
    """4 slots, 9 utterances (case 1's and one more)"""
    d, tensors, blob, dil = _mol11(oracle)
    m = make_model(4, dil, tensors, xcd_many=1)
    assert m.kernel_name() == "wn_xcd_many_kernel" and m.fused_conditioning()
    utts = _utterances(oracle, "mol11", d, blob, CASE1) + [_utterance(oracle, "mol11", d, blob, 8, 2)]
    _run_list(m, utts, chunk_frames=1, order="longest_first")


def test_one_stream_of_a_chain_workgroups_pair_restarts(torch_cuda, oracle):
    """the many-streams kernel gives chain workgroup c of XCD x the streams x + 8 * 2c and x + 8 * (2c + 1): a pair needs at least 9
    slots.  9 slots, the first ten utterances of the two-per-XCD case: behind chunk 0 slot 8 restarts, slot 0 -- the other stream of
    its chain workgroup, same service workgroup -- continues"""
    from twvk_amd import queue as Q
    lengths = CASE2[:10]
    p = Q.plan(lengths, 9, 1, "fifo")
    assert p.table[1, 8, Q.START] == 1 and p.table[1, 8, Q.UTT] == 9
    assert p.table[1, 0, Q.UTT] == p.table[0, 0, Q.UTT] == 0 and p.table[1, 0, Q.START] == 0
    d, tensors, blob, dil = _mol11(oracle)
    m = make_model(9, dil, tensors, xcd_many=1)
    assert m.kernel_name() == "wn_xcd_many_kernel"
    _run_list(m, _utterances(oracle, "mol11", d, blob, lengths, first_uid=20), chunk_frames=1, order="fifo")


# ---------------------------------------------------------------- 4. generic kernel, materialised conditioning
def test_list_on_the_generic_kernel(torch_cuda, oracle):
    """xcd = 0: eight workgroups per stream, each with its own copy of the stream's delay lines -- all eight blocks of a refilled
    slot are reset; the conditioning is upsampled and projected per chunk"""
    d, tensors, blob, dil = _mol11(oracle)
    m = make_model(3, dil, tensors, xcd=0)
    assert m.kernel_name() == "wn_generate_kernel" and not m.fused_conditioning()
    _run_list(m, _utterances(oracle, "mol11", d, blob, CASE1), chunk_frames=2, order="longest_first")
    _run_list(m, _utterances(oracle, "mol11", d, blob, CASE1), chunk_frames=1, order="fifo", check=False)


# ---------------------------------------------------------------- 5. wide kernel
def test_list_on_the_wide_kernel(torch_cuda, oracle):
    from twvk_amd.wavenet import WaveNetModel
    dil = [1, 2, 4, 8]
    d = oracle.make_dims(dil, R=64, D=64, S=512, Q=256, out_channels=30, scalar_input=True, ifw=32, use_bias=True, G=32, gc_card=2, L=80,
                         up=(5, 5, 12))
    tensors = shift_mol_head(dict(oracle.random_tensors(d, seed=0, scale=0.05)), 30)
    blob = oracle.blob_from_tensors(d, tensors)
    m = WaveNetModel(3, dil, 2, 64, 64, 512, quantization_channels=256, out_channels=30, use_biases=True, scalar_input=True,
                     initial_filter_width=32, global_condition_channels=32, global_condition_cardinality=2, local_condition_channels=80,
                     upsample_factor=[5, 5, 12], train_mode=False)
    m.load_weights(tensors)
    assert m.kernel_name() == "wn_wide_generate_kernel"
    _run_list(m, _utterances(oracle, "wide64", d, blob, [2, 1, 3, 1, 1, 2]), chunk_frames=1, order="fifo")


# ---------------------------------------------------------------- 6. one-hot mu-law model on the XCD kernel
def test_list_of_the_onehot_model(torch_cuda, oracle):
    """int32 class ids, float64 uniforms (padding 0.5 as a double), gc ids and seeds that differ per utterance"""
    dil = ([2 ** i for i in range(10)] * 2)[:11]
    d, tensors, blob = make_case(oracle, dil, scalar_input=False, S=512, Q=256, scale=0.12)
    m = make_model(3, dil, tensors, scalar_input=False, S=512, Q=256)
    assert m.kernel_name() == "wn_xcd_generate_kernel" and m.fused_conditioning()
    utts = _utterances(oracle, "onehot11", d, blob, [1, 2, 1, 3, 1, 2])
    assert len({x["gc"] for x in utts}) == 2 and len({int(x["seed"]) for x in utts}) > 2
    got = m.generate_list([x["mel"] for x in utts], [x["gc"] for x in utts], [x["seed"] for x in utts], [x["u"] for x in utts],
                          chunk_frames=2, order="longest_first")
    assert all(g.dtype == torch_cuda.int32 for g in got)
    _run_list(m, utts, chunk_frames=2, order="longest_first")
    _run_list(m, utts, chunk_frames=1, order="fifo", check=False)


# ---------------------------------------------------------------- 7. twv_wavenet_reset_streams by itself
@pytest.mark.parametrize("family", ["wn_xcd_generate_kernel", "wn_generate_kernel"])
def test_reset_streams_through_ctypes(torch_cuda, oracle, family):
    """B = 3: 300 steps, reset lane 1 only, 300 more.  Lanes 0 and 2 equal an uninterrupted 600 steps (two-frame utterances), lane 1
    a fresh model on its second utterance.  All-zero flags change no byte of the state; all-one flags are reset_state in effect"""
    torch = torch_cuda
    from twvk_amd import _lib
    d, tensors, blob, dil = _mol11(oracle)
    a, c = _utterance(oracle, "mol11", d, blob, 20, 2), _utterance(oracle, "mol11", d, blob, 21, 2)
    b1, b2 = _utterance(oracle, "mol11", d, blob, 28, 1), _utterance(oracle, "mol11", d, blob, 30, 1)
    m = make_model(3, dil, tensors, xcd=1 if family == "wn_xcd_generate_kernel" else 0)
    assert m.kernel_name() == family
    gc1, gc2 = [a["gc"], b1["gc"], c["gc"]], [a["gc"], b2["gc"], c["gc"]]
    mel1 = np.stack([a["mel"][:1], b1["mel"], c["mel"][:1]])
    mel2 = np.stack([a["mel"][1:], b2["mel"], c["mel"][1:]])
    u1 = np.stack([a["u"][:HOP], b1["u"], c["u"][:HOP]])
    u2 = np.stack([a["u"][HOP:], b2["u"], c["u"][HOP:]])
    seed1 = np.array([a["seed"], b1["seed"], c["seed"]], np.float32)
    want1 = np.stack([a["want"][:HOP], b1["want"], c["want"][:HOP]])
    want2 = np.stack([a["want"][HOP:], b2["want"], c["want"][HOP:]])

    def reset(flags):
        f = torch.tensor(flags, dtype=torch.int32, device=m.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(m._L.twv_wavenet_reset_streams(m._h, C.c_void_p(m._state.data_ptr()), 3, C.c_void_p(f.data_ptr()), stream))
        torch.cuda.synchronize()

    got1 = m.generate(m.create_upsample(mel1), gc1, seed1, u1).cpu().numpy()
    assert first_mismatch(got1, want1) is None, first_mismatch(got1, want1)
    before = m._state.clone()
    reset([0, 0, 0])
    assert torch.equal(m._state.view(torch.int32), before.view(torch.int32)), "all-zero flags must change nothing"
    reset([0, 1, 0])
    seed2 = np.array([got1[0, -1], b2["seed"], got1[2, -1]], np.float32)
    got2 = m.generate(m.create_upsample(mel2), gc2, seed2, u2).cpu().numpy()
    assert first_mismatch(got2, want2) is None, first_mismatch(got2, want2)
    reset([1, 1, 1])
    again = m.generate(m.create_upsample(mel1), gc1, seed1, u1).cpu().numpy()
    assert first_mismatch(again, want1) is None, first_mismatch(again, want1)
    assert m.status() == 0


# ---------------------------------------------------------------- 8. texts_to_waves
E2E_TOKENS = [[5, 9, 33, 12, 1], [7, 7, 1], [11, 40, 3, 62, 21, 8, 1], [30, 1], [17, 2, 55, 9, 44, 71, 28, 13, 1]]


def test_texts_to_waves_matches_chained_oracles(torch_cuda, oracle):
    """the geometry of tests/test_e2e_gpu.py (num_freq 65, a four-layer S = 64 vocoder on 2 slots), five utterances of differing
    input lengths through Tacotron in batches of two, each trimmed by the rule of synthesizer.py:232-256 and vocoded at its own
    length; against the oracle's Tacotron restatement (same batches, same padding) chained into its WaveNet restatement.
    max_iters is 7, not that file's 3: the focus of the monotonic attention never moves back, so the positions on `end` are the
    last ones of the decode and the rule can only cut through its quota of 5 -- which takes more than 6 decoder steps.  7 is the
    smallest decode at which one of these utterances (the two-token one) is cut earlier than the others"""
    import twvk_amd
    from twvk_amd.tacotron import Synthesizer
    from twvk_amd.e2e import texts_to_waves, attention_trim_frames
    hp = twvk_amd.default_hparams()
    hp.max_iters, hp.num_freq = 7, 65
    td = oracle.taco_dims(max_iters=7, num_freq=65)
    tt = oracle.taco_random_tensors(td, seed=5)
    syn = Synthesizer(); syn.load(tt, num_speakers=2, hparams=hp)
    dil = [1, 2, 4, 8]
    wd, wt, wblob = make_case(oracle, dil, S=64, shift=5.0)
    voc = make_model(2, dil, wt, S=64)
    assert voc.kernel_name() == "wn_generate_kernel" and not voc.fused_conditioning()
    spk = np.array([1, 0, 0, 1, 1], np.int32)
    # ---- oracle chain, Tacotron in the same batches of two
    mels, frames = [], []
    tblob = oracle.taco_blob(td, tt)
    for p in range(0, 5, 2):
        batch = E2E_TOKENS[p:p + 2]
        width = max(len(t) for t in batch)
        tok = np.zeros((len(batch), width), np.int32)
        for i, t in enumerate(batch):
            tok[i, :len(t)] = t
        mel_o, _, al_o = oracle.taco_infer(td, tblob, tok, np.array([len(t) for t in batch], np.int32), spk[p:p + 2])
        for i in range(len(batch)):
            keep = min(attention_trim_frames(al_o[i], width, hp.reduction_factor), mel_o.shape[1])
            mels.append(mel_o[i, :keep]); frames.append(keep)
    assert len(set(frames)) > 1, frames                                   # the trimmed lengths must not all be equal
    us, refs = [], []
    for i in range(5):
        U = oracle.upsample(wd, wblob, mels[i][None])
        u, ref = sensitive_mol(oracle, wd, wblob, U, spk[i:i + 1], np.zeros(1, np.float32), 1, frames[i] * HOP, seed=9 + i)
        us.append(u[0]); refs.append(ref[0])
    out = texts_to_waves(syn, voc, E2E_TOKENS, spk, us, attention_trim=True, chunk_frames=8)
    assert out["frames"] == frames and out["input_lengths"] == [len(t) for t in E2E_TOKENS]
    for i in range(5):
        assert first_mismatch(out["mel"][i].cpu().numpy(), mels[i]) is None, i
        got = out["audio"][i].cpu().numpy()
        assert got.shape == (frames[i] * HOP,)
        assert first_mismatch(got, refs[i]) is None, (i, first_mismatch(got, refs[i]))
    assert voc.status() == 0
    # a callable draws per utterance once the trimmed length is known
    out2 = texts_to_waves(syn, voc, E2E_TOKENS, spk, lambda i, n: us[i][:n * HOP], attention_trim=True, chunk_frames=5, order="fifo", check=False)
    for i in range(5):
        assert first_mismatch(out2["audio"][i].cpu().numpy(), refs[i]) is None, i
    assert voc.status() == 0
