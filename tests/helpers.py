"""shared builders for the parity tests: one config -> (oracle dims, oracle blob, product model)."""
import numpy as np

from sensitive_inputs import (assert_mol_inputs, assert_onehot_inputs, knife_edge_mol, knife_edge_onehot, narrow_logistic_uniforms,
                              shift_mol_head)


def make_case(O, dilations, scalar_input=True, S=512, Q=256, out_channels=30, ifw=32, use_bias=True, G=32, gc_card=2,
              L=80, up=(5, 5, 12), seed=0, scale=0.05, shift=0.0):
    d = O.make_dims(dilations, R=32, D=32, S=S, Q=Q, out_channels=out_channels, scalar_input=scalar_input, ifw=ifw,
                    use_bias=use_bias, G=G, gc_card=gc_card, L=L, up=up)
    tensors = O.random_tensors(d, seed=seed, scale=scale)
    if shift and scalar_input:
        tensors = shift_mol_head(tensors, out_channels, by=shift)     # narrow components: the samples leave the clamp
    blob = O.blob_from_tensors(d, tensors)
    return d, tensors, blob


def make_model(batch, dilations, tensors, scalar_input=True, S=512, Q=256, out_channels=30, ifw=32, use_bias=True, G=32,
               gc_card=2, L=80, up=(5, 5, 12), workers=None, groups=None, xcd=None, xcd_many=None):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    m = WaveNetModel(batch, dilations, 2, 32, 32, S, quantization_channels=Q, out_channels=out_channels,
                     use_biases=use_bias, scalar_input=scalar_input, initial_filter_width=ifw,
                     global_condition_channels=G or None, global_condition_cardinality=(gc_card or None) if G else None,
                     local_condition_channels=L or None, upsample_factor=list(up) if L else None, train_mode=False)
    if workers:
        m.set_option("workers", workers)
    if groups is not None:
        m.set_option("groups", groups)
    if xcd is not None:
        m.set_option("xcd", xcd)          # 0: the generic kernel even where the XCD-per-stream kernel qualifies
    if xcd_many is not None:
        m.set_option("xcd_many", xcd_many)  # 1: the many-streams XCD kernel (two streams per chain workgroup) also at batch <= 32
    m.load_weights(tensors)
    return m


def mol_uniforms(B, T, nr_mix, seed=2):
    rng = np.random.RandomState(seed)
    r = rng.random_sample((B, T, nr_mix + 1)).astype(np.float32)
    lo, hi = np.float32(1e-5), np.float32(1.0 - 1e-5)
    return (r * (hi - lo) + lo).astype(np.float32)   # tf.random_uniform(minval=1e-5, maxval=1-1e-5), mixture.py:103,110


def first_mismatch(a, b):
    a = np.asarray(a); b = np.asarray(b)
    bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
    return None if bad.size == 0 else tuple(int(v) for v in bad[0])


def builder_workers(d, B, T):
    """processes for the knife-edge builders: placing an edge costs about as much host time as the oracle's step, so long
    multi-stream cases deal their streams out (at most 16: the tests share a host)"""
    return min(B, 16) if B > 1 and B * T * d.n_layers >= 200000 else 1


def sensitive_mol(O, d, blob, U, gc, first_input, B, T, seed=2, prime=None):
    """(uniforms, the oracle's samples) for a MoL case whose point is sample equality: mol_uniforms (the logistic draw narrowed
    where the model has no bias to shift) with every mixture selection on its edge, and the conditions of
    tests/sensitive_inputs.py asserted on the oracle's output"""
    u0 = mol_uniforms(B, T, d.O // 3, seed)
    if not d.use_bias:
        u0 = narrow_logistic_uniforms(u0)
    u, want, n = knife_edge_mol(O, d, blob, U, gc, first_input, u0, prime, builder_workers(d, B, T))
    assert_mol_inputs(u, want, n)
    return u, want


def sensitive_onehot(O, d, blob, U, gc, first_input, u0, temperature=1.0, prime=None):
    """the one-hot counterpart: the plain draws u0 moved onto the class boundaries, conditions asserted"""
    B, T = np.shape(u0)
    u, want, n = knife_edge_onehot(O, d, blob, U, gc, first_input, u0, temperature, prime, builder_workers(d, B, T))
    assert_onehot_inputs(u, want, n, d.Q)
    return u, want


def assert_bar(label, got, g64, g32):
    """the gradient bar of tests/train_cases.py, per tensor of g64: max|got - g64| <= max(RATIO * max|g32 - g64|, FLOOR * max|g64|), finite
    and of g64's shape; prints every figure and returns the worst tensor as (name, e_got, e_g32)"""
    from train_cases import FLOOR, RATIO
    worst = ("", 0.0, 0.0)
    for k in g64:
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e_hip = float(np.abs(got[k].astype(np.float64) - g64[k]).max()) / scale
        e_t32 = float(np.abs(g32[k].astype(np.float64) - g64[k]).max()) / scale
        print("%s %-100s e_hip %.3e e_t32 %.3e ratio %6.2f%s" % (label, k, e_hip, e_t32, e_hip / max(e_t32, 1e-30), "  (floor)" if e_hip > RATIO * e_t32 else ""))
        assert np.isfinite(got[k]).all(), (label, k)
        assert got[k].shape == g64[k].shape, (label, k, got[k].shape, g64[k].shape)
        assert e_hip <= max(RATIO * e_t32, FLOOR), ("%s %s: HIP %.3g vs torch-f32 %.3g (relative to the tensor's max, against float64)" % (label, k, e_hip, e_t32))
        if e_hip > worst[1]:
            worst = (k, e_hip, e_t32)
    return worst


def same_outputs(a, b, what, skip=()):
    """two dicts of arrays hold the same bits (NaN equal to NaN), but for the keys of skip"""
    for k in a:
        if k not in skip:
            assert first_mismatch(a[k], b[k]) is None, (what, k, first_mismatch(a[k], b[k]))


def run_grad_handle(m, prefix, create_args, check_route, poison, call):
    """One run of a Tacotron gradient entry on a handle of its own: <prefix>_create(model, *create_args), check_route(the route label as a
    dict), a workspace filled with NaN (poison) or zeros, `call(g, ws, status, new)` -- which launches on the current stream and returns a
    dict of device tensors, its outputs made with new(*shape) so that they carry the same fill -- then synchronise and destroy the handle.
    Returns the dict as numpy arrays."""
    import ctypes as C
    import torch
    from twvk_amd import _lib
    L, dev, fill = m._L, m.device, float("nan") if poison else 0.0
    g = C.c_void_p()
    _lib.check(getattr(L, prefix + "_create")(m._h, *(tuple(create_args) + (C.byref(g),))))
    try:
        check_route(dict(kv.split("=", 1) for kv in getattr(L, prefix + "_route")(g).decode().split()))
        ws = torch.full((getattr(L, prefix + "_workspace_bytes")(g) // 4,), fill, dtype=torch.float32, device=dev)
        status = torch.zeros(4, dtype=torch.int32, device=dev)
        new = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            out = call(g, ws, status, new)
            torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    finally:
        getattr(L, prefix + "_destroy")(g)
