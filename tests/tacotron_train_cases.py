"""The case table of the Tacotron speaker-gradient and training-step tests (tests/test_tacotron_train_cpu.py proves the conditions on the
host, tests/test_tacotron_train_gpu.py runs the cases on the device).  Sizes are SMALL of tests/tacotron_grad_cases.py.

WHOLE: the two whole-model cases (tests/tacotron_cbhg_grad_cases.py's rows, seed overridden where given).  C-length-one is one of that
file's CHAIN_CASES and proved there.  F-speaker-tables (speaker_embedding_size 1) at its own seed 262 fails the chain conditions -- d
attention_g's float32 yardstick is 6.2e-6 of the tensor's maximum, above CHAIN_E_T32 -- and 263, the next seed, meets them all (relu
margin 2.4e-6, pool gap 3.6e-6, loss margin 3.7e-4, worst e_t32 7.2e-7); chosen on the CPU with HostCase(name, seed=...)."""
import functools

import numpy as np

from tacotron_cbhg_grad_cases import HostCase, hparams, SMALL      # noqa: F401

WHOLE = {"C-length-one": None, "F-speaker-tables": 263}

# speaker_grad in isolation: id -> (N, speaker ids, num_speakers, hparams overrides, seed)
SPEAKER_CASES = {
    "a-three": (3, (0, 1, 0), 2, {}, 301),
    "b-nine-unnamed-speaker": (9, (0, 1, 2, 2, 0, 1, 1, 0, 2), 4, {}, 302),      # (speaker 3 is named by no utterance)
    "c-one": (1, (1,), 2, {}, 303),
    "d-tables": (3, (0, 1, 0), 2, dict(speaker_embedding_size=1), 304),
    "e-tables-unnamed-speaker": (9, (0, 1, 2, 2, 0, 1, 1, 0, 2), 4, dict(speaker_embedding_size=1), 305),
    "f-one-layer": (3, (0, 1, 0), 2, dict(dec_layer_num=1), 306),
}

# the twenty-step run (test_tacotron_train_gpu.py): tacotron_initial_learning_rate and the schedule's mode; test_tacotron_train_cpu.py
# shows that twenty evaluation-graph steps of the float64 checker at this rate lower its own loss on C-length-one's batch
TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS = 1e-3, 1, 20


@functools.lru_cache(maxsize=None)
def whole_case(name):
    return HostCase(name, seed=WHOLE[name])


class SpeakerCase(object):
    """a model's weights, speaker ids and three host-made cotangents, scaled like d_memory of tests/tacotron_cbhg_grad_cases.py (1 / the
    number of rows)"""

    def __init__(self, name):
        import torch_attention_ref as AR
        from twvk_amd.tacotron import tacotron_specs
        self.name = name
        self.N, ids, self.speakers, kw, seed = SPEAKER_CASES[name]
        self.hp = hparams(max_iters=8, **dict(SMALL, **kw))
        self.specs = tacotron_specs(self.hp, self.speakers)
        self.w = AR.random_tensors(self.specs, seed=seed)
        self.dims = AR.Dims(self.hp, self.speakers)
        self.ids = np.asarray(ids, np.int32)
        rng = np.random.RandomState(seed + 1)
        hp = self.hp
        widths = (hp.enc_prenet_sizes[1], 2 * hp.enc_rnn_size, hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size)
        self.cot = [(rng.randn(self.N, n) / self.N).astype(np.float32) for n in widths]

    @functools.lru_cache(maxsize=None)
    def checker(self, dtype_name):
        import torch
        import torch_tacotron_speaker_grad_ref as SG
        return SG.speaker_vjp(self.w, self.dims, self.ids, self.cot[0], self.cot[1], self.cot[2], dtype=getattr(torch, dtype_name))


@functools.lru_cache(maxsize=None)
def speaker_case(name):
    return SpeakerCase(name)


@functools.lru_cache(maxsize=None)
def whole_checker(name, dtype_name):
    """(loss, grads, record) of SG.variable_vjp on a whole-model case"""
    import torch
    import torch_tacotron_speaker_grad_ref as SG
    h = whole_case(name)
    hp = h.hp
    return SG.variable_vjp(h.w, h.specs, h.dims, h.tok, h.ln, h.spk, h.at, h.tgt, h.lin_tgt, h.coeff, hp.prioritize_loss, hp.sample_rate,
                           hp.num_freq, dtype=getattr(torch, dtype_name))
