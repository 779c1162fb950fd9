"""The Tacotron feed on the device: twv_tacotron_batch_stage against prepare_batch bit for bit into NaN-filled outputs, and
gradient handles that follow the batch's shape -- one handle run through big -> small -> big -> another batch size against a handle newly
created at each stop, on NaN-filled workspaces, in every output bit for bit."""
import functools

import numpy as np
import pytest

from tacotron_feed_cases import NAMES, example, same_bits
from tacotron_grad_cases import SMALL, hparams

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the staging kernel
def _lengths(N, top_tokens, top_frames):
    """N (tokens, frames) pairs: the first fills (top_tokens, top_frames), then one frame, one token, and a spread"""
    rng = np.random.RandomState(N)
    pairs = [(top_tokens, top_frames), (max(top_tokens // 2, 1), 1), (1, max(top_frames // 3, 1))]
    while len(pairs) < N:
        pairs.append((int(rng.randint(1, top_tokens + 1)), int(rng.randint(1, top_frames + 1))))
    return pairs[:N]


def _stage(ex, M, F, t_in, t_out, shifts=(0, 0)):
    import torch
    from twvk_amd.tacotron_feed import ROW_DTYPE, ROW_WORDS, pack_batch, stage_packed
    buf, lay = pack_batch(ex, M, F, mel_shift=shifts[0], linear_shift=shifts[1])
    table = buf[lay["table_at"]:lay["table_at"] + ROW_WORDS * len(ex)].view(ROW_DTYPE).copy()
    dev = torch.from_numpy(buf.view(np.int32)).to("cuda:0")
    out = stage_packed(dev, table, lay, t_in, t_out, M, F, fill_nan=True)
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in NAMES}


STAGE_CASES = [(N, M, F) for N in (1, 3, 33) for M in (1, 80) for F in (1, 3, 1024, 1025)]


@pytest.mark.parametrize("N, M, F", STAGE_CASES)
def test_staging_equals_prepare_batch_bit_for_bit(N, M, F):
    """into outputs full of NaN / -1: an utterance that fills T_out exactly (T_out = its frames: the padded sizes are given, not
    prepare_batch's max + 1) and one that fills T_in, one of one frame and one of one token; then prepare_batch's own sizes; then T_out
    larger by several steps; then the mel and linear sections at odd words (every source alignment of the four-word vectors)"""
    from twvk_amd.tacotron_feed import prepare_batch
    r = 5
    rng = np.random.RandomState(100 * N + F + M)
    ex = [example(rng, nt, nf, M, F, n % 3, 0.25 * (n + 1)) for n, (nt, nf) in enumerate(_lengths(N, 11, 13))]
    want = prepare_batch(ex, r)
    t_in, t_out = want["inputs"].shape[1], want["mel_targets"].shape[1]
    assert (t_in, t_out) == (11, 15)

    def check(got, ti, to, what):
        for k in ("input_lengths", "loss_coeff", "speaker_id"):
            assert same_bits(got[k], want[k]), (what, k)
        for k, full in (("inputs", ti), ("mel_targets", to), ("linear_targets", to)):
            keep = min(full, want[k].shape[1])
            assert got[k].shape[1] == full and same_bits(got[k][:, :keep], want[k][:, :keep]), (what, k)
            assert not got[k][:, keep:].view(np.uint32).any(), (what, k, "padding")           # +0.0 / token 0, stored
            assert not want[k][:, keep:].any()
    check(_stage(ex, M, F, t_in, t_out), t_in, t_out, "prepare_batch's sizes")
    check(_stage(ex, M, F, 11, 13), 11, 13, "filled exactly")
    check(_stage(ex, M, F, t_in + 3, t_out + 4 * r), t_in + 3, t_out + 4 * r, "larger than needed")
    for shifts in ((1, 3), (3, 2), (2, 1)):
        check(_stage(ex, M, F, t_in, t_out, shifts), t_in, t_out, "odd sections %s" % (shifts,))


def test_staging_refuses_sizes_that_do_not_hold_the_batch():
    from twvk_amd._lib import TwvError
    rng = np.random.RandomState(0)
    ex = [example(rng, 4, 7, 3, 5), example(rng, 6, 2, 3, 5)]
    with pytest.raises(TwvError, match="twv_amd error 1: .*6 tokens do not fit t_in = 5"):
        _stage(ex, 3, 5, 5, 10)
    with pytest.raises(TwvError, match="twv_amd error 1: .*7 frames do not fit t_out = 6"):
        _stage(ex, 3, 5, 6, 6)


def test_stager_alternates_its_buffers_and_keeps_the_order():
    """five batches of different sizes through BatchStager, staged one ahead of their use: each is prepare_batch of its examples"""
    import torch
    from twvk_amd.tacotron_feed import BatchStager, prepare_batch
    M, F, r = 4, 1025, 5
    rng = np.random.RandomState(9)
    batches = [[example(rng, int(rng.randint(1, 12)), int(rng.randint(1, 30)), M, F, n % 2) for n in range(N)] for N in (3, 1, 5, 2, 4)]
    stager = BatchStager("cuda:0", M, F)
    staged = [stager.stage(b, r, wait=False) for b in batches]           # (all in flight before any is read: slots are reused twice)
    for b, s in zip(batches, staged):
        stager.ready(s)
        want = prepare_batch(b, r)
        for k in NAMES:
            assert same_bits(s[k].cpu().numpy(), want[k]), k
    torch.cuda.synchronize()


# ---------------------------------------------------------------- gradient handles that follow the shape
STOPS = ((4, 40, 8), (1, 1, 1), (4, 40, 8), (2, 23, 3))      # (N, T_in, steps): big (160 encoder and post rows: two 128-row chunks), smallest, big, another N
MAX_ITERS = 8


@functools.lru_cache(maxsize=None)
def _weights():
    import torch_attention_ref as AR
    from twvk_amd.tacotron import tacotron_specs
    hp = hparams(max_iters=MAX_ITERS, **SMALL)
    return hp, AR.random_tensors(tacotron_specs(hp, 2), seed=77)


def _model():
    from twvk_amd.tacotron import Tacotron
    hp, w = _weights()
    m = Tacotron(hp, num_speakers=2)
    m.load_weights(w)
    return m


def _inputs(stop, k):
    hp, _ = _weights()
    N, T, steps = stop
    rng = np.random.RandomState(1000 + k)
    TO = steps * hp.reduction_factor
    lengths = np.asarray([T] + [int(rng.randint(1, T + 1)) for _ in range(N - 1)], np.int32)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln:] = 0
    f = lambda *shape: rng.randn(*shape).astype(np.float32)
    return {"tok": tok, "ln": lengths, "spk": (np.arange(N) % 2).astype(np.int32), "tgt": f(N, TO, hp.num_mels), "d_mel": f(N, TO, hp.num_mels) / (N * TO),
            "d_memory": f(N, T, 2 * hp.enc_rnn_size) / (N * T), "d_linear": f(N, TO, hp.num_freq) / (N * TO)}


def _passes(m, stop, x, mode):
    """the three passes at `stop` on NaN-filled workspaces: every output, gradient and statistic as numpy, by name"""
    import torch
    hp = m._hparams
    N, T, steps = stop
    nan = float("nan")
    m.forward_targets(x["tok"], x["ln"], x["spk"], x["tgt"], teacher_forced=True)
    for kind, sizes in (("decoder", (N, T, steps)), ("encoder", (N, T)), ("post", (N, steps * hp.reduction_factor))):
        g, ws = m._grad_handle(kind, sizes)
        ws.fill_(nan)
        assert ws.numel() >= getattr(m._L, {"decoder": "twv_tacotron_decoder_grad"}.get(kind, "twv_tacotron_cbhg_grad") + "_workspace_bytes")(g) // 4
    out = {}
    grad, d_memory, d_init, mel = m._decoder_grad_blob(x["d_mel"])
    out.update({"dec.grad": grad, "dec.d_memory": d_memory, "dec.d_init": d_init, "dec.mel": mel})
    grad, memory, d_bh, d_ei = m._encoder_grad_blob(x["d_memory"], None, mode)
    out.update({"enc.grad": grad, "enc.memory": memory, "enc.d_bh": d_bh, "enc.d_init": d_ei})
    grad, d_mel, lin = m._postnet_grad_blob(x["d_linear"], x["tgt"], mode)
    out.update({"post.grad": grad, "post.d_mel": d_mel, "post.linear": lin})
    if mode == "batch":
        out["enc.stats"], out["post.stats"] = m._batch_stats_flat("encoder"), m._batch_stats_flat("post")
    if stop == (1, 1, 1):                                       # the post net alone at one row: T_out = 1 is no multiple of r
        g, ws = m._grad_handle("post", (1, 1))
        ws.fill_(nan)
        grad, d_mel, lin = m._postnet_grad_blob(x["d_linear"][:, :1], x["tgt"][:, :1], mode)
        out.update({"post1.grad": grad, "post1.d_mel": d_mel, "post1.linear": lin})
        if mode == "batch":
            out["post1.stats"] = m._batch_stats_flat("post")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("mode", ["inference", "batch"])
def test_a_reshaped_handle_gives_a_new_handles_bits(mode):
    one, fresh = _model(), _model()
    handles = {}
    for k, stop in enumerate(STOPS):
        x = _inputs(stop, k)
        got = _passes(one, stop, x, mode)
        fresh._drop_grad_handles()                              # (a handle created at this stop, as before this contract existed)
        want = _passes(fresh, stop, x, mode)
        assert set(got) == set(want) and len(got) >= 11
        for name in sorted(want):
            assert same_bits(got[name], want[name]), (stop, name)
            assert np.isfinite(want[name]).all(), (stop, name)
        assert all(want[n].any() for n in ("dec.grad", "enc.grad", "post.grad", "dec.d_memory", "dec.d_init", "post.d_mel"))
        # the same three handles all along, their workspaces never smaller
        now = {kind: (e[1].value, e[2].numel()) for kind, e in one._grad_cache.items()}
        for kind, (ptr, floats) in handles.items():
            assert now[kind][0] == ptr and now[kind][1] >= floats, kind
        handles = now
        assert one.decoder_grad_route() == fresh.decoder_grad_route() and one.cbhg_grad_route("post") == fresh.cbhg_grad_route("post")


def test_a_backward_straight_after_a_reshape_is_refused():
    import torch
    from twvk_amd._lib import TwvError
    from twvk_amd.tacotron import _ptr, _stream
    m = _model()
    x = _inputs(STOPS[0], 0)
    _passes(m, STOPS[0], x, "inference")
    hp = m._hparams
    N, T, steps = STOPS[3]
    g, ws = m._grad_handle("decoder", (N, T, steps))
    p, status = _ptr(m._blob), torch.zeros(4, dtype=torch.int32, device=m.device)
    L = m._L
    assert L.twv_tacotron_decoder_grad_backward(g, p, p, p, p, p, _ptr(ws), _ptr(status), _stream(), p, p, p) == 1
    assert "no forward has been made" in L.twv_last_error().decode()
    for kind, sizes, call in (("encoder", (N, T), lambda g, ws: L.twv_tacotron_encoder_grad_backward(g, p, p, p, p, _ptr(ws), _ptr(status), _stream(), p, p, p)),
                              ("post", (N, steps * hp.reduction_factor), lambda g, ws: L.twv_tacotron_postnet_grad_backward(g, p, p, p, _ptr(ws), _ptr(status), _stream(), p, p))):
        g, ws = m._grad_handle(kind, sizes)
        assert call(g, ws) == 1 and "no forward has been made" in L.twv_last_error().decode(), kind
    # the Python halves say the same: a forward at one shape, the handle reshaped, the backward refused
    m.forward_targets(x["tok"], x["ln"], x["spk"], x["tgt"], teacher_forced=True)
    m.encoder_grad_forward()
    m._grad_handle("encoder", (N, T))
    with pytest.raises(TwvError, match="no forward has been made"):
        m.encoder_grad_backward(x["d_memory"])
    # a refused reshape leaves the cached handle at its sizes
    before = m._grad_cache["decoder"]
    with pytest.raises(TwvError, match="steps must satisfy"):
        m._grad_handle("decoder", (N, T, MAX_ITERS + 1))
    assert m._grad_cache["decoder"] == before
    torch.cuda.synchronize()


def test_reserved_workspaces_are_not_allocated_again():
    m = _model()
    m.reserve_gradients(4, 40, 8)
    kept = {k: (e[2].data_ptr(), e[2].numel()) for k, e in m._grad_cache.items()}
    assert set(kept) == {"decoder", "encoder", "post"}
    for k, stop in enumerate(STOPS):
        _passes(m, stop, _inputs(stop, k), "inference")
        assert {k2: (e[2].data_ptr(), e[2].numel()) for k2, e in m._grad_cache.items()} == kept
    m._drop_grad_handles()                                      # the reservation outlives the handles
    g, ws = m._grad_handle("decoder", (1, 1, 1))
    assert ws.numel() == kept["decoder"][1]
