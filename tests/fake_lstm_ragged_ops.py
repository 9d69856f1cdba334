"""CPU restatement of the persistent recurrence WITH per-clip lengths (`ops.lstm_layer(..., lengths=)`, csrc/lstmseq.hip): paired
`fake_ops.lstm_step_pair` steps in which the state of every clip that is past its own length is forced to zero — by assignment, never by
a product, since `gates_x` may hold anything there.  `installed()` is `fake_ops.installed()` plus this one op."""
import contextlib

import torch

import fake_ops
from pantomatrix_amd import ops


def lstm_layer(dtype, gates_x, w_hh, w_scale, hseq, sync, *, a_scale=None, lengths=None):
    if lengths is None:
        return fake_ops.lstm_layer(dtype, gates_x, w_hh, w_scale, hseq, sync, a_scale=a_scale)
    assert fake_ops.lstm_layer_supported(dtype, hseq.shape[2] // 2) and sync.dtype == torch.int32
    b, t, h2 = hseq.shape
    hid = h2 // 2
    assert lengths.dtype == torch.int32 and lengths.shape == (b,)
    ln = lengths.long().clamp(0, t)
    mark = len(fake_ops.CALLS)
    cstate = torch.zeros(2, b, hid)
    prev = [torch.zeros(b, hid), torch.zeros(b, hid)]
    for s in range(t):
        sf, sb = s, t - 1 - s
        cur = [hseq[:, sf, :hid], hseq[:, sb, hid:]]
        fake_ops.lstm_step_pair(dtype, (prev[0], w_hh[0], gates_x[:, sf, :4 * hid], cstate[0], cur[0], w_scale[0]),
                                (prev[1], w_hh[1], gates_x[:, sb, 4 * hid:8 * hid], cstate[1], cur[1], w_scale[1]), a_scale=a_scale)
        for d, step in ((0, sf), (1, sb)):
            dead = ln <= step
            cstate[d][dead] = 0.0
            cur[d][dead] = 0.0
        prev = cur
    del fake_ops.CALLS[mark:]
    fake_ops.CALLS.append("lstm_layer_lengths")
    return hseq


@contextlib.contextmanager
def installed():
    with fake_ops.installed():
        saved = ops.lstm_layer
        ops.lstm_layer = lstm_layer
        try:
            yield
        finally:
            ops.lstm_layer = saved
