"""The case table of the Tacotron encoder / post-net gradient tests (tests/test_tacotron_cbhg_grad_cpu.py proves the margin condition for
every case on the host, tests/test_tacotron_cbhg_grad_gpu.py runs them on the device, scripts/tacotron_cbhg_grad_parity.py records them)
and the host-only inputs of a case.  Sizes are SMALL of tests/tacotron_grad_cases.py: bank sizes 4 and 3 cover even and odd kernel
widths and both sides of the SAME padding.

Every input of both C entries is made on the host, so that the float64 / float32 checker runs the CPU test compares are the ones the
device is held against: before_highway and the GRUs' initial states come from the checker's speaker side, the post net's input is the
float64 restatement's teacher-forced mel (rounded to float32) where T_out is a multiple of r, random frames otherwise.

The seeds were chosen on the CPU (scripts/tacotron_cbhg_grad_parity.py --seeds) so that the float64 and the float32 checker run take the
same branch at every relu and pool window, with the smallest |pre-activation| and pool gap above MARGIN."""
import functools

import numpy as np

from tacotron_grad_cases import R_, SMALL, hparams, padded_tokens      # noqa: F401 -- (the tests import SMALL and hparams from here)

# The device's row products accumulate in float64, so one of its pre-activations (of size ~1 here) differs from the exact one by the float32
# rounding of its inputs and of itself, a few 1e-7; a case's smallest |pre-activation| and pool gap must stay an order of magnitude clear of that.
MARGIN = 1e-6
# id -> (N, T_in, lengths, T_out, speakers, hparams overrides, encoder prenet masks, seed)
CASES = {
    "A-masked-tails": (3, 19, (19, 12, 7), 40, 2, {}, False, 216),
    "B-nine-utterances": (9, 23, (23, 20, 17, 14, 11, 8, 5, 23, 2), 10, 2, {}, False, 228),
    "C-length-one": (3, 19, (19, 1, 7), 15, 2, {}, False, 231),
    "D-one-row": (2, 1, (1, 1), 1, 2, {}, False, 241),
    "E-single-speaker": (3, 19, (19, 12, 7), 15, 1, {}, False, 254),
    "F-speaker-tables": (3, 19, (19, 12, 7), 15, 2, dict(speaker_embedding_size=1), False, 262),
    "G-bank-one-depth-one": (3, 19, (19, 12, 7), 15, 2, dict(enc_bank_size=1, post_bank_size=1, enc_highway_depth=1, post_highway_depth=1), False, 272),
    "H-odd-channels": (3, 19, (19, 12, 7), 15, 2, dict(enc_bank_channel_size=30, post_bank_channel_size=30, post_bank_size=4), False, 282),
    "I-dropout-masks": (3, 19, (19, 12, 7), 15, 2, {}, True, 293),
}

# The cases of the whole-model chain test (one 'deepvoice', one single-speaker).  Their whole-model checker runs are held to the margin
# condition too, and to CHAIN_E_T32: every tensor's float32 yardstick within 2e-6 of float64.  A tensor beyond that is a cancellation whose
# yardstick is noise, not a measure: at A-masked-tails' seed d attention_b has a maximum of 7e-6 (5e-4 at the neighbouring seeds) and its
# float32 autograd error moved between 1.4e-6 and 7.5e-6 from one host to another, with the device's decoder pass at 1.5e-5 of that maximum.
CHAIN_CASES = ("C-length-one", "E-single-speaker")
CHAIN_E_T32 = 2e-6


class HostCase(object):
    """weights and inputs of a case, numpy float32 / int32, host only"""

    def __init__(self, name, seed=None):
        import torch_attention_ref as AR
        import torch_tacotron_cbhg_grad_ref as CG
        import torch_tacotron_targets_ref as TR
        from twvk_amd.tacotron import tacotron_specs
        self.name = name
        self.N, self.T, lengths, self.TO, self.speakers, kw, with_masks, case_seed = CASES[name]
        seed = case_seed if seed is None else seed
        self.hp = hparams(max_iters=8, **dict(SMALL, **kw))
        self.at = self.hp.attention_type
        self.specs = tacotron_specs(self.hp, self.speakers)
        self.w = AR.random_tensors(self.specs, seed=seed)
        self.dims = AR.Dims(self.hp, self.speakers)
        self.enc_names, self.post_names = CG.encoder_names(self.specs), CG.postnet_names(self.specs)
        rng = np.random.RandomState(seed + 1)
        self.tok = padded_tokens(rng, self.N, self.T, lengths)
        self.ln = np.asarray(lengths, np.int32)
        self.spk = (np.arange(self.N) % 2).astype(np.int32)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        bh, ei, _ = CG.speaker_side(self.w, self.dims, self.spk)
        self.bh, self.init = f32(bh), f32(ei)
        P, M, F = self.hp.enc_prenet_sizes, self.hp.num_mels, self.hp.num_freq
        self.d_memory = (rng.randn(self.N, self.T, 2 * self.hp.enc_rnn_size) / (self.N * self.T)).astype(np.float32)
        self.masks = [(2.0 * rng.randint(0, 2, (self.N, self.T, d))).astype(np.float32) for d in P] if with_masks else None
        self.tgt = rng.uniform(-4.0, 4.0, (self.N, self.TO, M)).astype(np.float32)
        self.forced = self.TO % R_ == 0            # a teacher-forced device pass of this T_out exists
        if self.forced:
            self.mel = f32(TR.forward_targets(self.w, self.dims, self.tok, self.ln, self.spk, self.at, self.tgt, self.TO, True)[0])
        else:
            self.mel = rng.uniform(-4.0, 4.0, (self.N, self.TO, M)).astype(np.float32)
        self.d_linear = (rng.randn(self.N, self.TO, F) / (self.N * self.TO)).astype(np.float32)
        self.lin_tgt = rng.uniform(-4.0, 4.0, (self.N, self.TO, F)).astype(np.float32)
        self.coeff = rng.uniform(0.5, 2.0, self.N).astype(np.float32)

    @functools.lru_cache(maxsize=None)
    def encoder_checker(self, dtype_name):
        import torch
        import torch_tacotron_cbhg_grad_ref as CG
        return CG.encoder_vjp(self.w, self.enc_names, self.dims, self.tok, self.ln, self.bh, self.init, self.d_memory, self.masks,
                              dtype=getattr(torch, dtype_name))

    @functools.lru_cache(maxsize=None)
    def postnet_checker(self, dtype_name):
        import torch
        import torch_tacotron_cbhg_grad_ref as CG
        return CG.postnet_vjp(self.w, self.post_names, self.dims, self.mel, self.d_linear, dtype=getattr(torch, dtype_name))

    @functools.lru_cache(maxsize=None)
    def chain_checker(self, dtype_name):
        """the whole model from the tokens and the gradient of add_loss's loss: (loss, mel, linear, grads, record)"""
        import torch
        import torch_tacotron_cbhg_grad_ref as CG
        hp = self.hp
        return CG.loss_vjp(self.w, self.specs, self.dims, self.tok, self.ln, self.spk, self.at, self.tgt, self.lin_tgt, self.coeff, hp.prioritize_loss,
                           hp.sample_rate, hp.num_freq, dtype=getattr(torch, dtype_name))

    def margins(self):
        """(same branches on both sides?, smallest relu margin, smallest pool gap) of the float64 against the float32 checker run"""
        import torch_tacotron_cbhg_grad_ref as CG
        e64, e32, p64, p32 = (self.encoder_checker("float64")[2], self.encoder_checker("float32")[2], self.postnet_checker("float64")[2],
                              self.postnet_checker("float32")[2])
        return (CG.same_branches(e64, e32) and CG.same_branches(p64, p32), min(e64["relu_margin"], p64["relu_margin"]),
                min(e64["pool_gap"], p64["pool_gap"]))


@functools.lru_cache(maxsize=None)
def host_case(name):
    return HostCase(name)
