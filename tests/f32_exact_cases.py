"""Inputs of the per-op checks of the f32 parity mode (tests/test_f32_exact_cpu.py, tests/test_f32_exact_gpu.py): the operands
of one op, and a host-side stand-in for a context's weights (test infrastructure; no GPU).

- random set: FULL-MANTISSA f32 normals -- ReLU'd where the op reads a stored activation, signed for tensors read through an
  in-affine and for residuals; stem pixels are integers 0..255.  Short (bf16-valued) operands would make a product formed in f32
  exact and hide that mistake;
- dyadic set: the grids of test_conv_exact_gpu._dyadic_weights / _act(dyadic=True): every sum is exact in any order."""
import numpy as np
import torch

from test_conv_exact_gpu import _act, _dyadic_weights


def inputs(rng, g, o, n, dyadic):
    """{tensor id: NCHW float32 torch tensor, logical channels} for op o: everything it reads, and the concat buffer it
    writes a slice of"""
    def act(td, signed):
        if dyadic:
            return _act(rng, n, td, signed, True).float()
        x = rng.normal(0, 1, size=(n, td.channels_logical, td.height, td.width)).astype(np.float32)
        return torch.from_numpy(x if signed else np.maximum(x, 0))
    tin = g.tensors[o.in_]
    tens = {}
    if o.kind == 3:
        x = rng.integers(0, 256, size=(n, 4, tin.height, tin.width)).astype(np.float32)
        x[:, 3] = 0
        tens[o.in_] = torch.from_numpy(x)
    else:
        tens[o.in_] = act(tin, o.in_affine >= 0)
    if o.in2 >= 0:
        tens[o.in2] = act(g.tensors[o.in2], False)
    if o.res >= 0:
        tens[o.res] = act(g.tensors[o.res], True)
    if o.out >= 0 and o.out != o.in_ and g.tensors[o.out].channels_logical != g.layers[o.layer].cout:
        tens[o.out] = act(g.tensors[o.out], False)   # SSH concat slice: the untouched channels keep these
    return tens


class Weights:
    """get_layer / get_affine / set_layer / set_affine of a detector context, host-side.  Random: He-scaled normal weights with
    full f32 mantissas, affines of either sign."""

    def __init__(self, g, rng):
        self.w, self.b, self.aff = [], [], []
        for L in g.layers:
            fan = L.kh * L.kw * L.cin
            self.w.append(rng.normal(0, 1.4 / np.sqrt(fan), size=(L.cout, L.kh, L.kw, L.cin)).astype(np.float32))
            self.b.append(rng.normal(0, 0.1, size=L.cout).astype(np.float32))
            self.aff.append((rng.uniform(-0.2, 1.5, size=L.cout).astype(np.float32), rng.normal(0, 0.2, size=L.cout).astype(np.float32)))

    def get_layer(self, i, L):
        return self.w[i], self.b[i]

    def get_affine(self, i, cout):
        return self.aff[i]

    def set_layer(self, i, w, b):
        self.w[i], self.b[i] = np.asarray(w, np.float32), np.asarray(b, np.float32)

    def set_affine(self, i, s, t):
        self.aff[i] = (np.asarray(s, np.float32), np.asarray(t, np.float32))

    def dyadic(self, g, rng):
        _dyadic_weights(self, g, rng)
        return self
