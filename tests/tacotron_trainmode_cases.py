"""The case table of the Tacotron training-mode tests: batch-statistics batch norm in the encoder / post-net passes and the
training-mode step.  tests/test_tacotron_trainmode_cpu.py proves every case's conditions on the host, tests/test_tacotron_trainmode_gpu.py
runs the cases on the device, scripts/tacotron_trainmode_parity.py records them.  Sizes are SMALL of tests/tacotron_grad_cases.py.

The host inputs of a case are made as tests/tacotron_cbhg_grad_cases.py makes them (its HostCase, given this table's row), the checker runs
are tests/torch_tacotron_trainmode_ref.py's.  The seeds were chosen on the CPU (scripts/tacotron_trainmode_parity.py --seeds: the first
seed from the row's starting value) so that the float64 and the float32 checker run IN TRAINING MODE take the same branch at every relu
and pool window, with the smallest |pre-activation| and pool gap above MARGIN: the evaluation graph's seeds do not carry over (two of
that table's rows have a relu margin under 1e-6 once the batch norm takes the batch's statistics).

J-chunks crosses the column-statistics kernels' chunk of 128 rows with a ragged tail on both sides: 9 x 23 = 207 rows (two chunks) and
9 x 30 = 270 rows (three chunks, no multiple of 4).  K-one-row has R = N * T = 1 on both sides: every variance is 0 and every batch norm's
output is beta."""
import functools

import numpy as np

import tacotron_cbhg_grad_cases as CC
from tacotron_cbhg_grad_cases import MARGIN, SMALL, hparams      # noqa: F401

NINE = (23, 20, 17, 14, 11, 8, 5, 23, 2)
# id -> (N, T_in, lengths, T_out, speakers, hparams overrides, encoder prenet masks, seed)
CASES = {
    "A-masked-tails": (3, 19, (19, 12, 7), 40, 2, {}, False, 1218),
    "E-single-speaker": (3, 19, (19, 12, 7), 15, 1, {}, False, 1255),
    "F-speaker-tables": (3, 19, (19, 12, 7), 15, 2, dict(speaker_embedding_size=1), False, 1262),
    "G-bank-one-depth-one": (3, 19, (19, 12, 7), 15, 2, dict(enc_bank_size=1, post_bank_size=1, enc_highway_depth=1, post_highway_depth=1), False, 1272),
    "H-odd-channels": (3, 19, (19, 12, 7), 15, 2, dict(enc_bank_channel_size=30, post_bank_channel_size=30, post_bank_size=4), False, 1282),
    "I-dropout-masks": (3, 19, (19, 12, 7), 15, 2, {}, True, 1294),
    "J-chunks": (9, 23, NINE, 30, 2, {}, False, 1302),
    "K-one-row": (1, 1, (1,), 1, 2, {}, False, 1311),
}

# The whole-model cases of the training-mode step test, with dropout masks at all four sites from the device's generator (restated in
# numpy: tacotron.dropout_mask_numpy) under STEP_SEED at step 0.  Their seeds meet, besides the margin condition, the chain conditions of
# tests/tacotron_cbhg_grad_cases.py: loss margin above 1e-5, cumprod margin above 1e-3 and every tensor's float32 yardstick -- but the two
# proj_2 biases', whose gradient is exactly zero -- below CHAIN_E_T32.
# id -> (N, T_in, lengths, T_out, speakers, hparams overrides, seed)
# The float32 yardsticks of this graph fall with the number of rows the statistics are taken over: at three utterances (45 post-net rows)
# the worst of a run lies between 2.1e-6 and 1e-5 -- none of 300 seeds met CHAIN_E_T32 -- at nine (135 rows) two of the first eight do.
# 1501 is the first: relu margin 1.07e-6, worst yardstick 1.87e-6 (post_cbhg/highway_1/T/bias).
STEP_CASES = {
    "S-nine-deepvoice": (9, 23, NINE, 15, 2, {}, 1501),
}
# the batch of the twenty-step run (no comparison of gradients: the chain conditions are not asked of it)
TWENTY_CASES = {
    "U-three-deepvoice": (3, 19, (19, 1, 7), 15, 2, {}, 1408),
}
STEP_SEED = 7
CHAIN_E_T32 = CC.CHAIN_E_T32          # the evaluation graph's bound between a measure and noise holds here too
ZERO_GRADIENTS = ("encoder_cbhg/proj_2/conv1d/bias", "post_cbhg/proj_2/conv1d/bias")      # a constant in front of a batch norm is removed by it

# the twenty-step run: the rate and the schedule's mode of tests/tacotron_train_cases.py
TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS = 1e-3, 1, 20


class HostCase(CC.HostCase):
    """tests/tacotron_cbhg_grad_cases.py's HostCase on a row of this table, its checker runs in training mode: each returns
    (output, grads, record, statistics by name)"""

    def __init__(self, name, seed=None, table=None):
        row = (table or CASES)[name]
        CC.CASES["trainmode/" + name] = row         # (that class reads its row from its module's table)
        try:
            CC.HostCase.__init__(self, "trainmode/" + name, seed)
        finally:
            del CC.CASES["trainmode/" + name]
        self.name = name

    @functools.lru_cache(maxsize=None)
    def encoder_checker(self, dtype_name):
        import torch
        import torch_tacotron_trainmode_ref as TM
        return TM.encoder_vjp(self.w, self.enc_names, self.dims, self.tok, self.ln, self.bh, self.init, self.d_memory, self.masks,
                              dtype=getattr(torch, dtype_name))

    @functools.lru_cache(maxsize=None)
    def postnet_checker(self, dtype_name):
        import torch
        import torch_tacotron_trainmode_ref as TM
        return TM.postnet_vjp(self.w, self.post_names, self.dims, self.mel, self.d_linear, dtype=getattr(torch, dtype_name))

    def step_masks(self, step=0, seed=STEP_SEED):
        """the four dropout masks of a training-mode step from the generator's numpy restatement"""
        from twvk_amd.tacotron import dropout_mask_numpy
        hp = self.hp
        steps = self.TO // hp.reduction_factor
        shapes = [(self.N, self.T, hp.enc_prenet_sizes[0]), (self.N, self.T, hp.enc_prenet_sizes[1]), (self.N, steps, hp.dec_prenet_sizes[0]),
                  (self.N, steps, hp.dec_prenet_sizes[1])]
        return [dropout_mask_numpy(int(np.prod(s)), seed, step, site, 0.5).reshape(s) for site, s in enumerate(shapes)]

    @functools.lru_cache(maxsize=None)
    def chain_checker(self, dtype_name):
        """the whole model in training mode with step 0's masks: (loss, mel, linear, grads, record, statistics)"""
        import torch
        import torch_tacotron_trainmode_ref as TM
        hp = self.hp
        return TM.loss_vjp(self.w, self.specs, self.dims, self.tok, self.ln, self.spk, self.at, self.tgt, self.lin_tgt, self.coeff, hp.prioritize_loss,
                           hp.sample_rate, hp.num_freq, masks=self.step_masks(), dtype=getattr(torch, dtype_name))


def step_conditions(h):
    """(ok, figures) of a whole-model case: the margin and chain conditions of the float64 against the float32 run"""
    import torch_tacotron_cbhg_grad_ref as CG
    _, _, _, g64, rec, _ = h.chain_checker("float64")
    _, _, _, g32, rec32, _ = h.chain_checker("float32")
    worst = max((float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-30), k) for k in g64 if k not in ZERO_GRADIENTS)
    fig = dict(same=CG.same_branches(rec, rec32), relu_margin=rec["relu_margin"], pool_gap=rec["pool_gap"], loss_margin=rec["loss_margin"],
               cumprod_margin=rec["cumprod_margin"], worst_e_t32=worst[0], worst_tensor=worst[1])
    ok = (fig["same"] and fig["relu_margin"] > MARGIN and fig["pool_gap"] > MARGIN and fig["loss_margin"] > 1e-5 and fig["cumprod_margin"] > 1e-3
          and rec["min_one_minus_p"] >= np.finfo(np.float32).tiny and worst[0] < CHAIN_E_T32)
    return ok, fig


@functools.lru_cache(maxsize=None)
def host_case(name):
    return HostCase(name)


@functools.lru_cache(maxsize=None)
def step_case(name):
    N, T, lengths, TO, speakers, kw, seed = dict(STEP_CASES, **TWENTY_CASES)[name]
    return HostCase(name, table={name: (N, T, lengths, TO, speakers, kw, False, seed)})


@functools.lru_cache(maxsize=None)
def checker_trajectory(name, dtype_name="float64"):
    """TWENTY_STEPS training-mode steps of the checker on a case's fixed batch (gradients in `dtype_name`, the update in float64), masks of
    STEP_SEED at steps 0 .., randomly_initialized=False as tests/test_tacotron_train_gpu.py's twenty steps: (the losses before each
    update, the sum of |gradient| over every variable at the last of them)"""
    import torch
    import torch_tacotron_speaker_grad_ref as SG
    import torch_tacotron_trainmode_ref as TM
    h = step_case(name)
    hp = h.hp
    losses, _, g1 = TM.train_steps(h.w, h.specs, h.dims, (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff), lambda k: h.step_masks(step=k),
                                   lambda s: SG.learning_rate(TWENTY_LR0, s, TWENTY_MODE, False), hp.adam_beta1, hp.adam_beta2, TWENTY_STEPS,
                                   hp.prioritize_loss, hp.sample_rate, hp.num_freq, h.at, dtype=getattr(torch, dtype_name))
    return tuple(losses), g1
