"""TEST-ONLY stand-ins for the fused cross-attention sites (`ops.q_attention`, `ops.qm_attention`), restated with the CPU stand-ins of the
launches they replace (tests/fake_ops.py): the q projection, the stack's composed K / V launch, the attention.  Installed on top of
`fake_ops.installed()` by tests that force the sites' predicates on; the product has no switch that reaches this file."""
from __future__ import annotations

import contextlib

import torch

import fake_ops
from pantomatrix_amd import ops

D, T, H = 768, 64, 4
CALLS = []


def q_attention(dtype, a, w, bias, k, vt, vt_rows, out, b, *, w_scale, a_scale=None, ln=None, ln_eps=1e-5):
    CALLS.append(("q_attention", tuple(k.shape), vt_rows))
    q = torch.empty(b * T, D)
    fake_ops.gemm(dtype, a, w, bias, out_f32=q, n=D, cp=D, w_scale=w_scale, a_scale=a_scale, ln=ln, ln_eps=ln_eps)
    fake_ops.attention(dtype, q, k, vt, vt_rows, out, b, H, T, T, D // H)


def qm_attention(dtype, a, w, bias, mem, wkv, bias_kv, kv_layers, kv_layer, out, b, *, w_scale, wkv_scale, a_scale=None, ln=None, ln_eps=1e-5):
    CALLS.append(("qm_attention", tuple(mem.shape), int(wkv.shape[1]), kv_layers, kv_layer))
    n = kv_layers * D
    k, vt = torch.empty(b * T, n), torch.zeros(b, n, T)
    fake_ops.gemm(dtype, mem, wkv, bias_kv, out_f32=k, out_t=vt, n=2 * n, cp=int(wkv.shape[1]), t_col0=n, t_rows=T, w_scale=wkv_scale, a_scale=a_scale)
    q = torch.empty(b * T, D)
    fake_ops.gemm(dtype, a, w, bias, out_f32=q, n=D, cp=D, w_scale=w_scale, a_scale=a_scale, ln=ln, ln_eps=ln_eps)
    fake_ops.attention(dtype, q, k[:, kv_layer * D:(kv_layer + 1) * D], vt[:, kv_layer * D:], n, out, b, H, T, T, D // H)


@contextlib.contextmanager
def installed():
    saved = (ops.q_attention, ops.qm_attention)
    with fake_ops.installed():
        try:
            ops.q_attention, ops.qm_attention = q_attention, qm_attention
            CALLS.clear()
            yield
        finally:
            ops.q_attention, ops.qm_attention = saved
