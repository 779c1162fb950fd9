"""The checker of the Tacotron encoder and post-net gradients (twv_tacotron_encoder_grad_run / twv_tacotron_postnet_grad_run /
twv_tacotron_linear_loss_grad, Tacotron.loss_gradients): tests/torch_tacotron_ref.py `_cbhg` restated on that module's own helpers WITHOUT
no_grad and differentiated by autograd.  Test infrastructure only.

Two things differ from `_cbhg`, neither in the forward value: the max pool is `torch.where(later > earlier, later, earlier)`, so that
autograd sends the whole cotangent of a tie to the EARLIER position (TensorFlow's MaxPoolGrad as recalled; torch.maximum splits a tie), and
every relu's pre-activation and every pool window's pair are looked at on the way, for the run's margins: the smallest |pre-activation| at
any relu, the smallest gap |x_t - x_{t+1}| at the pool that is no tie, and the branch taken at each (`record["branches"]`), so that a float64 and
a float32 run can be shown to have taken the same ones -- a comparison across a flipped branch means nothing.

float64 is the checker, float32 the yardstick (tests/train_cases.py RATIO / FLOOR); `_as_dtype` is torch_tacotron_grad_ref's switch.
A batch_normalization leaf is the (4, C) checkpoint tensor; its gradient is reported as (2, C) = (d_gamma, d_beta)."""
import numpy as np
import torch

import torch_attention_ref as AR
import torch_tacotron_grad_ref as G
import torch_tacotron_ref as R

GP = G.GP
TIE_GAP = 1e-10          # float64 pool values (of size ~1) closer than this are equal up to summation order: see _max_pool2


def encoder_names(specs):
    return [n for n, _ in specs if n == "embedding" or n.startswith("prenet/") or n.startswith("encoder_cbhg/")]


def postnet_names(specs):
    names = [n for n, _ in specs]
    return [n for n in names if n.startswith("post_cbhg/")] + names[-2:]


def model_names(specs):
    """every tensor Tacotron.loss_gradients differentiates: all but the speaker table and its dense layers"""
    return encoder_names(specs) + G.decoder_names(specs) + postnet_names(specs)


def new_record():
    return {"cumprod_margin": float("inf"), "min_one_minus_p": float("inf"), "clamp_engaged": False,
            "relu_margin": float("inf"), "pool_gap": float("inf"), "loss_margin": float("inf"), "branches": []}


def _relu(z, rec):
    with torch.no_grad():
        rec["relu_margin"] = min(rec["relu_margin"], float(z.abs().min()))
        rec["branches"].append((z > 0).numpy().copy())
    return torch.relu(z)


def _max_pool2(x, rec):
    """max_pooling1d(2, strides 1, 'same'): the window of t is {t, t + 1}, padding never wins; a tie goes to the earlier position"""
    later = torch.cat([x[:, 1:], torch.full_like(x[:, :1], -float("inf"))], dim=1)
    take_later = later > x
    with torch.no_grad():
        # Two rows deep inside an utterance's padding see the same inputs, so their values are equal up to the summation order of the
        # library product that made them (~1e-16 in float64): a tie in all but name, harmless like an exact one (equal rows give equal
        # terms to every sum the cotangent enters).  Gaps at that level are not margins, and their windows not branches to compare.
        gap = torch.cat([(x[:, :-1] - x[:, 1:]).abs(), torch.full_like(x[:, :1], float("inf"))], dim=1)
        tie = gap <= TIE_GAP
        if bool((~tie & torch.isfinite(gap)).any()):
            rec["pool_gap"] = min(rec["pool_gap"], float(gap[~tie & torch.isfinite(gap)].min()))
        rec["branches"].append(np.ma.masked_array(take_later.numpy().copy(), mask=tie.numpy().copy()))
    return torch.where(take_later, later, x)


def _conv_block(x, w, scope, relu, rec):
    y = R._conv1d_same(x, R._t(w[scope + "/conv1d/kernel"]), R._t(w[scope + "/conv1d/bias"]))
    if relu:
        y = _relu(y, rec)
    return R._batch_norm_inference(y, w[scope + "/batch_normalization"])


def _cbhg(x, lengths, w, scope, bank_size, n_proj, depth, before_highway=None, rnn_init=None, rec=None):
    """torch_tacotron_ref._cbhg, the same operations in the same order"""
    rec = new_record() if rec is None else rec
    bank = torch.cat([_conv_block(x, w, "%s/conv_bank/conv1d_%d" % (scope, k), True, rec) for k in range(1, bank_size + 1)], dim=-1)
    y = _max_pool2(bank, rec)
    for i in range(n_proj):
        y = _conv_block(y, w, "%s/proj_%d" % (scope, i + 1), i < n_proj - 1, rec)
    hw = y + x
    if before_highway is not None:
        hw = hw + before_highway[:, None, :]
    if scope + "/dense/kernel" in w:
        hw = R._dense(hw, w, scope + "/dense")
    for i in range(depth):
        p = "%s/highway_%d" % (scope, i + 1)
        H = _relu(R._dense(hw, w, p + "/H"), rec)
        T_ = R._dense(hw, w, p + "/T", torch.sigmoid)
        hw = H * T_ + hw * (1.0 - T_)
    fw = bw = None
    if rnn_init is not None:
        n = rnn_init.shape[1] // 2
        fw, bw = rnn_init[:, :n], rnn_init[:, n:]
    return R._bidirectional_gru(hw, lengths, w, scope, fw, bw)


def _leaves(w, names, dtype, want):
    return {k: torch.tensor(np.asarray(w[k]), dtype=dtype, requires_grad=want) for k in names}


def _leaf(a, dtype, want):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=want)


def _grad_of(t, name=""):
    g = t.grad if t.grad is not None else torch.zeros_like(t)
    return (g[:2] if name.endswith("batch_normalization") else g).numpy().copy()


def _encoder(wt, dims, tokens, lengths, bh, init, masks, rec, dtype):
    table = torch.cat([torch.zeros_like(wt["embedding"][:1]), wt["embedding"][1:]], dim=0)     # tacotron.py:53-56: the <PAD> row is zeros
    x = table[torch.as_tensor(np.asarray(tokens), dtype=torch.long)]
    h = _relu(R._dense(x, wt, "prenet/dense_1"), rec)
    if masks is not None:
        h = h * torch.as_tensor(np.asarray(masks[0]), dtype=dtype)
    h = _relu(R._dense(h, wt, "prenet/dense_2"), rec)
    if masks is not None:
        h = h * torch.as_tensor(np.asarray(masks[1]), dtype=dtype)
    return _cbhg(h, np.asarray(lengths), wt, "encoder_cbhg", dims.enc_bank, 2, dims.enc_hw_depth, bh, init, rec)


def encoder_vjp(w, names, dims, tokens, lengths, before_highway=None, rnn_init=None, d_memory=None, masks=None, dtype=torch.float64):
    """tokens -> memory and its vector-Jacobian product with d_memory (None: forward only).  Returns (memory, grads, record); grads maps
    `names` (encoder_names) plus "d_before_highway" / "d_rnn_init" where those inputs are given."""
    rec = new_record()
    want = d_memory is not None
    with G._as_dtype(dtype, rec), torch.set_grad_enabled(want):
        wt = _leaves(w, names, dtype, want)
        bh, init = _leaf(before_highway, dtype, want), _leaf(rnn_init, dtype, want)
        memory = _encoder(wt, dims, tokens, lengths, bh, init, masks, rec, dtype)
        grads = {}
        if want:
            memory.backward(torch.as_tensor(np.asarray(d_memory), dtype=dtype))
            grads = {k: _grad_of(wt[k], k) for k in names}
            if bh is not None:
                grads["d_before_highway"] = _grad_of(bh)
            if init is not None:
                grads["d_rnn_init"] = _grad_of(init)
    return memory.detach().numpy(), grads, rec


def postnet_vjp(w, names, dims, mel, d_linear=None, dtype=torch.float64):
    """mel -> linear and its vector-Jacobian product with d_linear.  Returns (linear, grads, record); grads maps `names` (postnet_names)
    plus "d_mel"."""
    rec = new_record()
    want = d_linear is not None
    with G._as_dtype(dtype, rec), torch.set_grad_enabled(want):
        wt = _leaves(w, names, dtype, want)
        m = _leaf(mel, dtype, want)
        post = _cbhg(m, None, wt, "post_cbhg", dims.post_bank, 2, dims.post_hw_depth, rec=rec)
        linear = R._dense(post, wt, names[-2][:-len("/kernel")])
        grads = {}
        if want:
            linear.backward(torch.as_tensor(np.asarray(d_linear), dtype=dtype))
            grads = {k: _grad_of(wt[k], k) for k in names}
            grads["d_mel"] = _grad_of(m)
    return linear.detach().numpy(), grads, rec


def _loss_terms(mel, linear, mel_t, lin_t, coeff, prioritize_loss, sample_rate, num_freq):
    """torch_tacotron_targets_ref.add_loss's lines on tensors: (mel term, linear term) of `loss`"""
    c = coeff[:, None, None]
    mel_l = (mel_t - mel).abs()
    l1 = (lin_t - linear).abs()
    if prioritize_loss:
        upper = int(5000 / (sample_rate * 0.5) * num_freq)
        lower = int(165 / (sample_rate * 0.5) * num_freq)
        pr = l1[:, :, lower:upper]
        return (mel_l * c).mean(), 0.5 * (l1 * c).mean() + 0.5 * (pr * c).mean()
    return (mel_l * c).mean(), (l1 * c).mean()


def linear_loss_cotangent(linear, linear_targets, loss_coeff, prioritize_loss, sample_rate, num_freq, dtype=torch.float64):
    """d(linear term of add_loss) / d linear by autograd of the loss lines"""
    lin = torch.tensor(np.asarray(linear), dtype=dtype, requires_grad=True)
    lt = torch.as_tensor(np.asarray(linear_targets), dtype=dtype)
    co = torch.as_tensor(np.asarray(loss_coeff), dtype=dtype)
    _, term = _loss_terms(torch.zeros(lin.shape[0], lin.shape[1], 1, dtype=dtype), lin, torch.zeros(lin.shape[0], lin.shape[1], 1, dtype=dtype),
                          lt, co, prioritize_loss, sample_rate, num_freq)
    term.backward()
    return lin.grad.numpy()


def speaker_side(w, dims, speaker_ids, dtype=torch.float64):
    """(before_highway, encoder_rnn_init, decoder_init) of a multi-speaker model as numpy in `dtype` -- the front of
    torch_tacotron_targets_ref.forward_targets (deepvoice with a speaker embedding, or the five tables of speaker_embedding_size 1) --
    or (None, None, None) for a single speaker"""
    if dims.n_speakers <= 1:
        return None, None, None
    with G._as_dtype(dtype, new_record()), torch.no_grad():
        ids = torch.as_tensor(np.asarray(speaker_ids), dtype=torch.long)
        if "speaker_embedding" not in w:
            tabs = ["before_highway", "encoder_rnn_init_state", "attention_rnn_init_state"] + ["decoder_rnn_init_states%d" % (i + 1) for i in range(dims.dec_layers)]
            v = [R._t(w[t])[ids] for t in tabs]
        else:
            spk = R._t(w["speaker_embedding"])[ids]
            softsign = lambda t: t / (t.abs() + 1.0)
            v = [R._dense(spk, w, "dense" if i == 0 else "dense_%d" % i, softsign) for i in range(3 + dims.dec_layers)]
        return v[0].numpy(), v[1].numpy(), torch.cat(v[2:], dim=1).numpy()


def _decoder(wt, dims, mem, init, lengths, attention_type, mel_targets, dtype):
    """torch_tacotron_grad_ref.decoder_vjp's lines on tensors: the teacher-forced decoder from (memory, decoder_init) to mel"""
    tg = np.asarray(mel_targets)
    N, t_out, M = tg.shape
    RR = dims.r
    steps = t_out // RR
    fed = torch.as_tensor(tg[:, RR - 1::RR, :], dtype=dtype)
    T_in = mem.shape[1]
    mask = torch.as_tensor(np.arange(T_in)[None, :] < np.asarray(lengths)[:, None])
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
        p = R._dense(p, wt, "decoder/decoder_prenet/dense_2", torch.relu)
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
    return torch.cat(mel_steps, dim=1)


def loss_vjp(w, specs, dims, tokens, lengths, speaker_ids, attention_type, mel_targets, linear_targets, loss_coeff, prioritize_loss,
             sample_rate, num_freq, dtype=torch.float64):
    """the whole model from the tokens, teacher-forced, and the gradient of add_loss's `loss`: returns (loss, mel, linear, grads, record);
    grads maps model_names(specs) plus "d_init" and, for a multi-speaker model, "d_before_highway" / "d_encoder_rnn_init" (the speaker
    side itself is not differentiated).  record["loss_margin"]: the smallest |output - target| (where the sign of a difference decides)."""
    names = model_names(specs)
    rec = new_record()
    N = np.asarray(tokens).shape[0]
    bh_np, ei_np, di_np = speaker_side(w, dims, speaker_ids, dtype)
    with G._as_dtype(dtype, rec):
        wt = _leaves(w, names, dtype, True)
        bh, ei = _leaf(bh_np, dtype, True), _leaf(ei_np, dtype, True)
        AS = wt["decoder/attention_wrapper/gru_cell/candidate/bias"].shape[0]
        DR = wt[GP + "cell_1/gru_cell/candidate/bias"].shape[0]
        di = _leaf(di_np if di_np is not None else np.zeros((N, AS + dims.dec_layers * DR)), dtype, True)
        memory = _encoder(wt, dims, tokens, lengths, bh, ei, None, rec, dtype)
        mel = _decoder(wt, dims, memory, di, lengths, attention_type, mel_targets, dtype)
        post = _cbhg(mel, None, wt, "post_cbhg", dims.post_bank, 2, dims.post_hw_depth, rec=rec)
        linear = R._dense(post, wt, postnet_names(specs)[-2][:-len("/kernel")])
        mt, lt = torch.as_tensor(np.asarray(mel_targets), dtype=dtype), torch.as_tensor(np.asarray(linear_targets), dtype=dtype)
        a, b = _loss_terms(mel, linear, mt, lt, torch.as_tensor(np.asarray(loss_coeff), dtype=dtype), prioritize_loss, sample_rate, num_freq)
        loss = a + b
        with torch.no_grad():
            rec["loss_margin"] = min(float((mel - mt).abs().min()), float((linear - lt).abs().min()))
        loss.backward()
        grads = {k: _grad_of(wt[k], k) for k in names}
        grads["d_init"] = _grad_of(di)
        if bh is not None:
            grads["d_before_highway"], grads["d_encoder_rnn_init"] = _grad_of(bh), _grad_of(ei)
    return float(loss.detach()), mel.detach().numpy(), linear.detach().numpy(), grads, rec


def same_branches(rec_a, rec_b):
    """did two runs of one case take the same branch at every relu and make the same choice at every pool window?"""
    a, b = rec_a["branches"], rec_b["branches"]
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        keep = ~np.ma.getmaskarray(x)                # (the pool windows that are ties in `rec_a`, the float64 run, are not compared)
        if not np.array_equal(np.ma.getdata(x)[keep], np.ma.getdata(y)[keep]):
            return False
    return True
