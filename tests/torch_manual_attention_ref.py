"""float64 restatement of the inference graph fed `is_manual_attention: True, manual_alignments: ...` (tacotron/tacotron.py:122-123): at
decoder step t the attention wrapper uses manual_alignments[:, t, :] in place of what its mechanism computes (rnn_wrappers.py:369-374).
Test infrastructure only: the checker of Tacotron.infer_manual.

The graph is tests/torch_attention_ref.py's `infer`, imported and not copied: its loop asks one object for `(alignments, next_state) =
mechanism(query, state)` and does everything else -- prenet, attention cell, context, projection, residual cells, post net -- itself.
`infer_manual` below runs that loop with the object replaced by one that ignores query and state and hands out the caller's rows step by
step, and with max_iters = the number of rows.  Nothing of the mechanism is computed, so no attention tensor of `w` is read (they may be
missing), the alignments are used exactly as given (no mask, no normalisation), and fed the alignments `infer` itself computed it performs
the same torch operations in the same order on the same values and returns the same float64 bits (tests/test_tacotron_manual_cpu.py).
"""
import copy

import numpy as np
import torch

import torch_attention_ref as AR


class _Injected(object):
    """stands in for torch_attention_ref._Mechanism: step k's alignments are manual[:, k, :], whatever the query and the state"""

    def __init__(self, manual):
        self.manual, self.k = manual, 0

    def initial_state(self, N, T_in):
        return torch.zeros(N, T_in, dtype=AR.F64)

    def __call__(self, query, state):
        align = self.manual[:, self.k, :].contiguous()             # (a tensor of its own, laid out as a mechanism's result is)
        self.k += 1
        return align, align                                        # (previous_alignments <- the manual row; nothing reads it)


@torch.no_grad()
def infer_manual(w, dims, tokens, lengths, speaker_ids, manual_alignments):
    """manual_alignments (N, steps, T_in) -> (mel (N, steps * r, M), linear, alignments (N, T_in, steps)) float64 numpy"""
    manual = torch.as_tensor(np.asarray(manual_alignments, np.float64))
    N, T_in = np.asarray(tokens).shape
    assert manual.dim() == 3 and manual.shape[0] == N and manual.shape[2] == T_in and manual.shape[1] >= 1, tuple(manual.shape)
    d = copy.copy(dims)
    d.max_iters = int(manual.shape[1])
    injected = _Injected(manual)
    mechanism = AR._Mechanism
    AR._Mechanism = lambda attention_type, w_, keys, mask: injected
    try:
        out = AR.infer(w, d, tokens, lengths, speaker_ids, "manual")
    finally:
        AR._Mechanism = mechanism
    assert injected.k == d.max_iters
    return out
