"""The case table of the decoder gradients at the softmax attention types and loc_sen (twv_tacotron_decoder_grad_create_any;
tests/test_tacotron_attention_grad_gpu.py runs the cases on the device, scripts/tacotron_attention_grad_parity.py records them and, with
--seeds, proves the table's conditions on the host).  The inputs of a case are made as tests/tacotron_grad_cases.py HostCase makes them
(that class reads its own module's table, so its constructor is restated here on this one), with one addition: the scores are sharpened.

With torch_attention_ref.random_tensors as it is, the softmax is almost flat (the largest alignment of a 19-position utterance is 0.055
against a uniform 1/19), and a flat softmax hides mistakes in its backward.  So every case scales ONE tensor by `sharpen`:
  bah, loc_sen           attention_v / attention_variable
  bah_norm               attention_g  (the normalised score reads v only through v / |v|: scaling attention_v changes nothing)
  luong, luong_scaled    memory_layer/kernel
The factor and the seed of each case were chosen on the host so that, in the float64 checker (scripts/tacotron_attention_grad_parity.py
--seeds; the figures are in profiles/tacotron_attention_grad_parity.txt):
  1. no gradient tensor is identically zero (but decoder_prenet/dense_1/kernel in a ONE-step case: the only frame fed is the all-zero go
     frame, so that kernel's gradient is zero whatever the weights),
  2. every tensor's float32-run distance e_t32 is at most 1e-4 (otherwise 8 x e_t32 bounds nothing),
  3. for every utterance longer than three positions the largest alignment over all steps lies in [0.2, 0.98].
conditions() measures the three; tests/test_tacotron_attention_grad_cpu.py asserts them for the smallest case of each kind."""
import numpy as np

from tacotron_grad_cases import R_, SMALL, hparams, padded_tokens

TAILS = (3, 19, (19, 12, 7))          # masked tails; lengths 12 and 7 are shorter than loc_sen's 15-tap half window
# id -> (attention_type, N, T_in, lengths, steps, hparams overrides, masks, seed, sharpen)
CASES = {
    "bah_norm-tails": ("bah_norm",) + TAILS + (8, {}, False, 133, 12.0),
    "bah-tails": ("bah",) + TAILS + (8, {}, False, 133, 12.0),
    "luong-tails": ("luong",) + TAILS + (8, {}, False, 131, 3.0),
    "luong_scaled-tails": ("luong_scaled",) + TAILS + (8, {}, False, 131, 3.0),
    "loc_sen-tails": ("loc_sen",) + TAILS + (8, {}, False, 131, 6.0),
    "bah_norm-length-one": ("bah_norm", 3, 19, (19, 1, 7), 4, {}, False, 172, 12.0),
    "bah-one-step": ("bah",) + TAILS + (1, {}, False, 164, 12.0),
    "luong_scaled-one-layer": ("luong_scaled",) + TAILS + (4, dict(dec_layer_num=1), False, 182, 3.0),
    "loc_sen-attention-128": ("loc_sen",) + TAILS + (4, dict(attention_size=128), False, 191, 6.0),
    "luong-nine-utterances": ("luong", 9, 23, (23, 20, 17, 14, 11, 8, 5, 23, 2), 5, {}, False, 154, 3.0),
    "bah_norm-dropout-masks": ("bah_norm",) + TAILS + (8, {}, True, 133, 12.0),
    "loc_sen-cumulative": ("loc_sen", 2, 40, (40, 33), 12, {}, False, 142, 6.0),
    # T_in just above 512: every thread owns two positions of the softmax (a Bahdanau type: see the docstring of the parity script)
    "bah_norm-two-positions-a-thread": ("bah_norm", 2, 530, (530, 301), 3, {}, False, 202, 48.0),
}
SHARPENED = {"bah_norm": "attention_g", "bah": "attention_v", "loc_sen": "attention_variable", "luong": "memory_layer/kernel",
             "luong_scaled": "memory_layer/kernel"}


class HostCase(object):
    """weights and inputs of a case, numpy float32 / int32, host only (memory and the initial states come from a device pass, or from
    encoder_side() on the host)"""

    def __init__(self, name, seed=None, sharpen=None):
        import torch_attention_ref as AR
        import torch_tacotron_grad_ref as G
        from twvk_amd.tacotron import tacotron_specs
        self.name = name
        self.at, self.N, self.T, lengths, self.steps, kw, with_masks, seed0, sharpen0 = CASES[name]
        seed = seed0 if seed is None else seed
        self.seed, self.sharpen = seed, sharpen0 if sharpen is None else sharpen
        self.hp = hparams(max_iters=max(self.steps, 8), **dict(SMALL, attention_type=self.at, **kw))
        self.specs = tacotron_specs(self.hp, 2)
        self.w = AR.random_tensors(self.specs, seed=seed)
        hit = [n for n, _ in self.specs if n == SHARPENED[self.at] or n.endswith("/" + SHARPENED[self.at])]
        assert len(hit) == 1, hit
        self.w[hit[0]] = (self.w[hit[0]] * np.float32(self.sharpen)).astype(np.float32)
        self.dims, self.names = AR.Dims(self.hp, 2), G.decoder_names(self.specs)
        rng = np.random.RandomState(seed + 1)
        self.tok = padded_tokens(rng, self.N, self.T, lengths)
        self.ln = np.asarray(lengths, np.int32)
        self.spk = (np.arange(self.N) % 2).astype(np.int32)
        M, TO = self.hp.num_mels, self.steps * R_
        self.tgt = rng.uniform(-4.0, 4.0, (self.N, TO, M)).astype(np.float32)
        self.d_mel = (rng.randn(self.N, TO, M) / (self.N * TO * M)).astype(np.float32)
        self.masks = None
        if with_masks:          # dropout at keep_prob 0.5: multipliers 0 or 2
            self.masks = [(2.0 * rng.randint(0, 2, (self.N, self.steps, d))).astype(np.float32) for d in self.hp.dec_prenet_sizes]

    def encoder_side(self):
        """(memory, decoder_init) float32 from the float64 restatement of the encoder: what a host-only run feeds the checker"""
        import torch_tacotron_grad_ref as G
        mem, init = G.encoder_side(self.w, self.dims, self.tok, self.ln, self.spk)
        return mem.astype(np.float32), init.astype(np.float32)

    def conditions(self):
        """the three conditions of the module docstring, measured in the checker on encoder_side(): (names of identically-zero gradient
        tensors, the worst tensor's (e_t32, name), the largest alignment of each utterance over all steps and its own positions)"""
        import torch
        import torch_attention_ref as AR
        import torch_tacotron_grad_ref as G
        mem, init = self.encoder_side()
        args = (self.w, self.names, self.dims, mem, init, self.ln, self.at, self.tgt, self.d_mel, self.masks)
        seen, call = [], AR._Mechanism.__call__

        def recording(mech, query, state):
            out = call(mech, query, state)
            seen.append(out[0].detach().numpy().copy())
            return out
        AR._Mechanism.__call__ = recording
        try:
            _, g64, _ = G.decoder_vjp(*args)
        finally:
            AR._Mechanism.__call__ = call
        _, g32, _ = G.decoder_vjp(*args, dtype=torch.float32)
        zero = [k for k in g64 if not g64[k].any() and not (self.steps == 1 and k == "decoder/decoder_prenet/dense_1/kernel")]
        e = [(float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-300), k) for k in g64]
        al = np.stack(seen)                 # (steps, N, T_in)
        return zero, max(e), [float(al[:, n, :ln].max()) for n, ln in enumerate(self.ln)]


def conditions_hold(case, zero, worst, amax):
    return not zero and worst[0] <= 1e-4 and all(0.2 <= a <= 0.98 for a, ln in zip(amax, case.ln) if ln > 3)


# ---- the whole model (tests/test_tacotron_attention_train_gpu.py): tokens -> loss, one case per new kind, shaped as
# tests/tacotron_cbhg_grad_cases.py's A-masked-tails.  id -> (attention_type, seed, sharpen).  Beside the three conditions above, the
# float64 and the float32 checker run take the same branch at every relu and pool window with the margins of
# tests/tacotron_cbhg_grad_cases.py MARGIN (whole_conditions, asserted by the test itself; scripts/tacotron_attention_grad_parity.py --seeds
# prints the figures).
WHOLE = {"whole-bah_norm": ("bah_norm", 406, 24.0), "whole-luong_scaled": ("luong_scaled", 411, 3.0), "whole-loc_sen": ("loc_sen", 421, 6.0)}
WHOLE_SHAPE = (3, 19, (19, 12, 7), 15, 2)          # N, T_in, lengths, T_out, speakers


class WholeCase(object):
    """weights and inputs of a whole-model case, numpy float32 / int32, host only; the fields tests/tacotron_cbhg_grad_cases.py HostCase
    gives the whole-model tests (that class reads its own module's table)"""

    def __init__(self, name, seed=None, sharpen=None, **hparams_kw):
        import torch_attention_ref as AR
        from twvk_amd.tacotron import tacotron_specs
        self.name = name
        self.at, seed0, sharpen0 = WHOLE[name]
        self.N, self.T, lengths, self.TO, self.speakers = WHOLE_SHAPE
        self.seed, self.sharpen = seed0 if seed is None else seed, sharpen0 if sharpen is None else sharpen
        self.hp = hparams(max_iters=8, **dict(SMALL, attention_type=self.at, **hparams_kw))
        self.specs = tacotron_specs(self.hp, self.speakers)
        self.w = AR.random_tensors(self.specs, seed=self.seed)
        hit = [n for n, _ in self.specs if n == SHARPENED[self.at] or n.endswith("/" + SHARPENED[self.at])]
        assert len(hit) == 1, hit
        self.w[hit[0]] = (self.w[hit[0]] * np.float32(self.sharpen)).astype(np.float32)
        self.dims = AR.Dims(self.hp, self.speakers)
        rng = np.random.RandomState(self.seed + 1)
        self.tok = padded_tokens(rng, self.N, self.T, lengths)
        self.ln = np.asarray(lengths, np.int32)
        self.spk = (np.arange(self.N) % 2).astype(np.int32)
        M, F = self.hp.num_mels, self.hp.num_freq
        self.tgt = rng.uniform(-4.0, 4.0, (self.N, self.TO, M)).astype(np.float32)
        self.lin_tgt = rng.uniform(-4.0, 4.0, (self.N, self.TO, F)).astype(np.float32)
        self.coeff = rng.uniform(0.5, 2.0, self.N).astype(np.float32)

    def checker(self, dtype_name):
        """(loss, grads, record) of torch_tacotron_speaker_grad_ref.variable_vjp"""
        import torch
        import torch_tacotron_speaker_grad_ref as SG
        hp = self.hp
        return SG.variable_vjp(self.w, self.specs, self.dims, self.tok, self.ln, self.spk, self.at, self.tgt, self.lin_tgt, self.coeff,
                               hp.prioritize_loss, hp.sample_rate, hp.num_freq, dtype=getattr(torch, dtype_name))

    def whole_conditions(self):
        """(all hold?, figures): no zero tensor, worst e_t32 <= 1e-4, the largest alignments in [0.2, 0.98], and the float64 and float32
        runs on the same side of every relu and pool window with margins above tacotron_cbhg_grad_cases.MARGIN"""
        import torch_attention_ref as AR
        import torch_tacotron_cbhg_grad_ref as CG
        from tacotron_cbhg_grad_cases import MARGIN
        seen, call = [], AR._Mechanism.__call__

        def recording(mech, query, state):
            out = call(mech, query, state)
            seen.append(out[0].detach().numpy().copy())
            return out
        AR._Mechanism.__call__ = recording
        try:
            _, g64, r64 = self.checker("float64")
        finally:
            AR._Mechanism.__call__ = call
        _, g32, r32 = self.checker("float32")
        zero = [k for k in g64 if not g64[k].any()]
        worst = max((float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-300), k) for k in g64)
        al = np.stack(seen)
        amax = [float(al[:, n, :ln].max()) for n, ln in enumerate(self.ln)]
        same = CG.same_branches(r64, r32)
        ok = (conditions_hold(self, zero, worst, amax) and same and r64["relu_margin"] > MARGIN and r64["pool_gap"] > MARGIN)
        return ok, dict(zero=zero, worst_e_t32=worst, largest_alignments=amax, same_branches=same, relu_margin=r64["relu_margin"], pool_gap=r64["pool_gap"])
