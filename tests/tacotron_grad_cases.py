"""The case table of the Tacotron decoder gradient tests (tests/test_tacotron_grad_gpu.py runs them on the device,
scripts/tacotron_grad_parity.py records them) and the host-only inputs of a case.  Default decoder widths, small encoder / post banks
(SMALL, also the sizes of tests/tacotron_cbhg_grad_cases.py): bank sizes 4 and 3 cover even and odd kernel widths and both sides of the
SAME padding."""
import numpy as np

R_ = 5
SMALL = dict(enc_bank_size=4, post_bank_size=3, num_freq=129)
# id -> (N, T_in, lengths, steps, hparams overrides, masks, seed)
CASES = {
    "A-masked-tails": (3, 19, (19, 12, 7), 8, {}, False, 131),
    "B-clamp": (2, 40, (40, 33), 12, {}, False, 141),
    "C-nine-utterances": (9, 23, (23, 20, 17, 14, 11, 8, 5, 23, 2), 5, {}, False, 151),
    "D-one-step": (3, 19, (19, 12, 7), 1, {}, False, 161),
    "E-length-one": (3, 19, (19, 1, 7), 4, {}, False, 171),
    "F-one-layer": (3, 19, (19, 12, 7), 4, dict(dec_layer_num=1), False, 181),
    "G-bah_mon": (3, 19, (19, 12, 7), 4, dict(attention_type="bah_mon"), False, 191),
    "H-dropout-masks": (3, 19, (19, 12, 7), 8, {}, True, 131),
}


def hparams(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def padded_tokens(rng, N, T, lengths):
    """random symbols, <EOS> (1) at each length, <PAD> (0) past it"""
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1
        tok[n, ln:] = 0
    return tok


class HostCase(object):
    """weights and inputs of a case, numpy float32 / int32, host only (memory and the initial states come from a device pass)"""

    def __init__(self, name):
        import torch_attention_ref as AR
        import torch_tacotron_grad_ref as G
        from twvk_amd.tacotron import tacotron_specs
        self.name = name
        self.N, self.T, lengths, self.steps, kw, with_masks, seed = CASES[name]
        self.hp = hparams(max_iters=max(self.steps, 8), **dict(SMALL, **kw))
        self.at = self.hp.attention_type
        self.specs = tacotron_specs(self.hp, 2)
        self.w = AR.random_tensors(self.specs, seed=seed)
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
