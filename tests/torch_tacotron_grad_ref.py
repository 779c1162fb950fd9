"""The checker of the Tacotron decoder gradients (twv_tacotron_decoder_grad_run): the teacher-forced decoder loop of
tests/torch_tacotron_targets_ref.py `forward_targets` (lines 81-100) WITHOUT no_grad, on the same imported helpers (torch_tacotron_ref's
_dense / _gru_cell / _monotonic_attention_parallel, torch_attention_ref's _Mechanism), differentiated by autograd.  Test infrastructure only.

Leaves: every decoder-side weight tensor (memory_layer/kernel .. decoder/output_projection_wrapper/bias), `memory` (the encoder output) and
`decoder_init` (the attention cell's initial state, then each residual GRU's).  Optional multipliers after the two decoder-prenet relus
(dropout masks) and the two monotonic attention types.  float64 is the checker; the float32 run of the same lines is the yardstick the HIP
gradients are held against (tests/train_cases.py RATIO / FLOOR).

The helpers cast through their module-level F64; `_as_dtype` points that name at the run's dtype for the run's duration, so the float32
run really is float32."""
import contextlib

import numpy as np
import torch

import torch_attention_ref as AR
import torch_tacotron_ref as R

FIRST, LAST = "memory_layer/kernel", "decoder/output_projection_wrapper/bias"
GP = "decoder/output_projection_wrapper/multi_rnn_cell/"


def decoder_names(specs):
    """names of the decoder-side tensors of a spec list, in blob order"""
    names = [n for n, _ in specs]
    return names[names.index(FIRST):names.index(LAST) + 1]


@contextlib.contextmanager
def _as_dtype(dtype, record):
    """helpers compute in `dtype`; every monotonic step's (p_choose, cumprod) margins go to `record`"""
    old = (R.F64, AR.F64, R._monotonic_attention_parallel)

    def recording(p_choose, previous):
        with torch.no_grad():
            cp = R._safe_cumprod_exclusive(1.0 - p_choose)
            record["cumprod_margin"] = min(record["cumprod_margin"], float(((cp - 1e-10).abs() / 1e-10).min()))
            record["min_one_minus_p"] = min(record["min_one_minus_p"], float((1.0 - p_choose).min()))
            record["clamp_engaged"] = record["clamp_engaged"] or bool((cp < 1e-10).any())
        return old[2](p_choose, previous)
    R.F64 = AR.F64 = dtype
    R._monotonic_attention_parallel = recording
    try:
        yield
    finally:
        R.F64, AR.F64, R._monotonic_attention_parallel = old


def encoder_side(w, dims, tokens, lengths, speaker_ids, dtype=torch.float64):
    """what the decoder reads from the encoder side, numpy in `dtype`: memory (N, T_in, 2 * enc_rnn) -- the encoder CBHG output, zero past
    each length -- and decoder_init (N, AS + layers * DR); the front of torch_tacotron_targets_ref.forward_targets, the same operations in
    the same order (deepvoice multi-speaker with speaker_embedding_size != 1, or a single speaker)"""
    with _as_dtype(dtype, {"cumprod_margin": 0.0, "min_one_minus_p": 0.0, "clamp_engaged": False}), torch.no_grad():
        return _encoder_side(w, dims, tokens, lengths, speaker_ids)


def _encoder_side(w, dims, tokens, lengths, speaker_ids):
    tokens = np.asarray(tokens); lengths = np.asarray(lengths)
    w = {k: R._t(v) for k, v in w.items()}
    N = tokens.shape[0]
    table = R._t(w["embedding"]).clone()
    table[0] = 0.0
    x = table[torch.as_tensor(tokens, dtype=torch.long)]
    AS = w["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
    DR = w[GP + "cell_1/gru_cell/candidate/bias"].shape[0]
    before_highway = enc_init = None
    if dims.n_speakers > 1:
        assert "speaker_embedding" in w and "dense_1/kernel" in w, "deepvoice multi-speaker models only"
        spk = R._t(w["speaker_embedding"])[torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)]
        softsign = lambda v: v / (v.abs() + 1.0)
        names = ["dense"] + ["dense_%d" % i for i in range(1, 3 + dims.dec_layers)]
        before_highway = R._dense(spk, w, names[0], softsign)
        enc_init = R._dense(spk, w, names[1], softsign)
        init = torch.cat([R._dense(spk, w, names[2 + i], softsign) for i in range(1 + dims.dec_layers)], dim=1)
    else:
        init = torch.zeros(N, AS + dims.dec_layers * DR, dtype=R.F64)
    h = R._dense(x, w, "prenet/dense_1", torch.relu)
    h = R._dense(h, w, "prenet/dense_2", torch.relu)
    enc = R._cbhg(h, lengths, w, "encoder_cbhg", dims.enc_bank, 2, dims.enc_hw_depth, before_highway, enc_init)
    return enc.numpy(), init.numpy()


def decoder_vjp(w, names, dims, memory, decoder_init, lengths, attention_type, mel_targets, d_mel=None, masks=None, dtype=torch.float64):
    """the teacher-forced decoder on (memory, decoder_init) and its vector-Jacobian product with d_mel (None: forward only).
    Returns (mel (N, T_out, M), grads, record) as numpy in `dtype`; grads maps every name of `names` plus "d_memory" and "d_init";
    record holds the clamp margins of the run (see _as_dtype)."""
    lengths = np.asarray(lengths)
    tg = np.asarray(mel_targets)
    N, t_out, M = tg.shape
    RR = dims.r
    assert t_out % RR == 0 and t_out >= RR and M == dims.num_mels
    steps = t_out // RR
    record = {"cumprod_margin": float("inf"), "min_one_minus_p": float("inf"), "clamp_engaged": False}
    want = d_mel is not None
    with _as_dtype(dtype, record), torch.set_grad_enabled(want):
        wt = {k: torch.tensor(np.asarray(w[k]), dtype=dtype, requires_grad=want) for k in names}
        mem = torch.tensor(np.asarray(memory), dtype=dtype, requires_grad=want)
        init = torch.tensor(np.asarray(decoder_init), dtype=dtype, requires_grad=want)
        fed = torch.as_tensor(tg[:, RR - 1::RR, :], dtype=dtype)
        T_in = mem.shape[1]
        mask = torch.as_tensor(np.arange(T_in)[None, :] < lengths[:, None])
        values = mem * mask[:, :, None].to(dtype)
        keys = values @ R._t(wt["memory_layer/kernel"])
        mech = AR._Mechanism(attention_type, wt, keys, mask)
        AS = wt["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
        DR = wt[GP + "cell_1/gru_cell/candidate/bias"].shape[0]
        att_h = init[:, :AS]
        dec_h = [init[:, AS + i * DR:AS + (i + 1) * DR] for i in range(dims.dec_layers)]
        context = torch.zeros(N, mem.shape[2], dtype=dtype)
        state = mech.initial_state(N, T_in)
        frame = torch.zeros(N, M, dtype=dtype)
        mel_steps = []
        for time in range(steps):
            p = R._dense(frame, wt, "decoder/decoder_prenet/dense_1", torch.relu)
            if masks is not None:
                p = p * torch.as_tensor(np.asarray(masks[0])[:, time], dtype=dtype)
            p = R._dense(p, wt, "decoder/decoder_prenet/dense_2", torch.relu)
            if masks is not None:
                p = p * torch.as_tensor(np.asarray(masks[1])[:, time], dtype=dtype)
            att_h = R._gru_cell(torch.cat([p, context], dim=-1), att_h, wt, "decoder/attention_wrapper/gru_cell")
            align, state = mech(att_h, state)
            context = (align[:, None, :] @ values)[:, 0]
            y = R._dense(torch.cat([att_h, context], dim=-1), wt, GP + "cell_0/output_projection_wrapper")
            for i in range(dims.dec_layers):
                dec_h[i] = R._gru_cell(y, dec_h[i], wt, GP + "cell_%d/gru_cell" % (i + 1))
                y = y + dec_h[i]
            out = R._dense(y, wt, "decoder/output_projection_wrapper")
            mel_steps.append(out.reshape(N, RR, M))
            frame = fed[:, time, :]
        mel = torch.cat(mel_steps, dim=1)
        grads = {}
        if want:
            mel.backward(torch.as_tensor(np.asarray(d_mel), dtype=dtype))
            for k in names:
                grads[k] = (wt[k].grad if wt[k].grad is not None else torch.zeros_like(wt[k])).numpy()
            grads["d_memory"], grads["d_init"] = mem.grad.numpy(), init.grad.numpy()
    return mel.detach().numpy(), grads, record
