"""f64 per-op reference with a per-element verdict (test infrastructure; pure torch / numpy, no GPU).

Evaluates ONE op of the graph in float64 from the bf16 inputs and the weights / bias / affine the device holds, and returns,
for every output element, the set of values the op may legally store:

- every sum of products is exact in f64 here (bf16 x bf16 products need 16 bits, sums of a few thousand of them far less than 53);
- the device sums in f32, in some order.  Its error is bounded statistically by r = 16 * 2^-24 * sqrt(K * sum_k (a_k b_k)^2)
  (computed by one more f64 conv of x^2 with w^2; K counts both K segments), and every f32 epilogue step (bias, residual,
  affine product and sum) widens the interval by its own rounding, 2^-24 |value|.  The interval goes through every rounding
  point (relu, max-pool and affines are monotone; a negative scale swaps the ends), and a bf16 output may be any value from
  RNE(lo) to RNE(hi).  An element is "decided" when that is one value;
- with `radius=False` the interval is the point v64 (the dyadic input set, whose f32 sums are exact in any order): every
  element must then be RNE(v64), bit for bit.  `exact=True` also asserts that every f64 intermediate is representable in f32,
  i.e. that the claim "exact in any order" really holds for the data.

RNE = round to nearest, ties to even, to bf16, of the f64 value itself (never through f32: no double rounding)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # f32 unit round-off: |RN(x) - x| <= U |x|


def rne_bf16(x):
    """f64 tensor -> f64 tensor of the nearest-even bf16 values (8 significant bits)."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), (e - 8).to(torch.float64))


def bf16_ties(x):
    """(ties rounded down in magnitude, ties rounded up) among the f64 values x, for RNE to bf16."""
    m, e = torch.frexp(x.abs())
    t = m * 256.0
    tie = (t - torch.floor(t)) == 0.5
    up = torch.round(t) > t
    return int((tie & ~up).sum()), int((tie & up).sum())


def grid_exponent(x, emax=40):
    """smallest e >= 0 with every x * 2^e an integer (asserts there is one up to emax)."""
    x = x.abs()
    for e in range(emax + 1):
        y = x * 2.0 ** e
        if bool((y == torch.floor(y)).all()):
            return e
    raise AssertionError("values are not on a dyadic grid of step >= 2^-%d" % emax)


class Out:
    """One output tensor of an op: [lo, hi] (bf16 outputs: already RNE'd ends), the exact centre v64, the raw (un-rounded)
    radius, and `dst`: logical channel of the device tensor for every output channel (SSH concat slices)."""

    def __init__(self, lo, hi, v, rad, is_f32=False, dst=None, softmax=False):
        self.lo, self.hi, self.v, self.rad, self.is_f32, self.dst, self.softmax = lo, hi, v, rad, is_f32, dst, softmax


def _cat(outs):
    """the Outs of consecutive image chunks of one tensor, as one Out"""
    a = outs[0]
    return Out(*(torch.cat([getattr(o, k) for o in outs]) for k in ("lo", "hi", "v", "rad")), is_f32=a.is_f32, dst=a.dst, softmax=a.softmax)


class ExactRef:
    def __init__(self, graph, det):
        self.g = graph
        self.w, self.b, self.aff = [], [], []
        for i, L in enumerate(graph.layers):
            w, b = det.get_layer(i, L)
            self.w.append(torch.from_numpy(w).permute(0, 3, 1, 2).contiguous().double())  # [cout][cin][kh][kw]
            self.b.append(torch.from_numpy(b).double())
            if L.has_affine:
                s, t = det.get_affine(i, L.cout)
                self.aff.append((torch.from_numpy(s).double(), torch.from_numpy(t).double()))
            else:
                self.aff.append(None)
        self.radius = True
        self.exact = False

    # ---- interval steps (lo, hi, v: f64 tensors) ----
    def _f32(self, lo, hi, v):
        """one f32 rounding of the value"""
        if self.exact:
            assert torch.equal(v.float().double(), v), "dyadic set: an intermediate is not exact in f32"
        if not self.radius:
            return lo, hi, v
        return lo - U * lo.abs(), hi + U * hi.abs(), v

    def _add(self, lo, hi, v, c):
        return self._f32(lo + c, hi + c, v + c)

    def _affine(self, lo, hi, v, s, t):
        """v * s (rounded) + t (rounded), per channel; a negative scale swaps the ends"""
        s, t = s.view(1, -1, 1, 1), t.view(1, -1, 1, 1)
        a, b = lo * s, hi * s
        lo, hi, v = self._f32(torch.minimum(a, b), torch.maximum(a, b), v * s)
        return self._add(lo, hi, v, t)

    @staticmethod
    def _relu(lo, hi, v):
        return lo.clamp_min(0), hi.clamp_min(0), v.clamp_min(0)

    @staticmethod
    def _bf16(lo, hi, v):
        return rne_bf16(lo), rne_bf16(hi), v

    def _acc(self, segs, stride=1, pad=0, groups=1):
        """f64 sum over K segments [(x, w, stride)], and the accumulation radius"""
        s = q = None
        k = 0
        for x, w, st in segs:
            c = F.conv2d(x, w, None, stride=st, padding=pad, groups=groups)
            s = c if s is None else s + c
            if self.radius:
                c2 = F.conv2d(x * x, w * w, None, stride=st, padding=pad, groups=groups)
                q = c2 if q is None else q + c2
            k += w.shape[1] * w.shape[2] * w.shape[3]
            pad = 0  # the second segment is an unpadded 1x1 conv
        r = 16.0 * U * torch.sqrt(k * q) if self.radius else torch.zeros_like(s)
        return s, r

    def _operand(self, x, s, t):
        """bf16(relu(x * s + t)): the producer's affine applied to a conv operand -> (value, width of its legal set)"""
        lo, hi, v = self._affine(x, x, x, s, t)
        lo, hi, v = self._bf16(*self._relu(lo, hi, v))
        return rne_bf16(v), hi - lo

    # ---- ops ----
    def run_op(self, i, tens, chunk=0):
        """tens: dict tensor id -> NCHW f64 tensor (bf16 values; logical channels).  Returns {tensor id: Out} for every
        output of op i except out_b of a back-to-back op (b2b_second: it reads the device's own stored first output).
        chunk > 0: evaluated `chunk` images at a time (every op treats the images of a batch independently) and concatenated,
        so the f64 intermediates of a 16-image chain on the 160 x 160 maps never exist all at once."""
        n = next(iter(tens.values())).shape[0]
        if chunk <= 0 or chunk >= n:
            return self._run_op(i, tens)
        parts = [self._run_op(i, {t: x[k:k + chunk] for t, x in tens.items()}) for k in range(0, n, chunk)]
        return {t: _cat([p[t] for p in parts]) for t in parts[0]}

    def _run_op(self, i, tens):
        g = self.g
        o = g.ops[i]
        L = g.layers[o.layer]
        x = tens[o.in_]
        res = {}
        if o.kind in (0, 5, 3):  # conv0 7x7/2 | first 3x3/2 on R,G,B (+ stem: max-pool 3x3/2 pad 1, affine, relu)
            pad = 3 if o.kind != 5 else 1
            xs = x[:, :3]
            self._check_exact([(xs, self.w[o.layer], 2)], self.b[o.layer], L.kh, pad)
            s, r = self._acc([(xs, self.w[o.layer], 2)], pad=pad)
            lo, hi, v = self._add(s - r, s + r, s, self.b[o.layer].view(1, -1, 1, 1))
            lo, hi, v = self._bf16(*self._relu(lo, hi, v))
            if o.kind == 3:
                v = rne_bf16(v)   # the stored conv0 output: the pool reads bf16 values
                lo, hi, v = (F.max_pool2d(z, 3, 2, 1) for z in (lo, hi, v))
                sc, sh = self.aff[o.layer]
                lo, hi, v = self._bf16(*self._relu(*self._affine(lo, hi, v, sc, sh)))
            res[o.out] = Out(lo, hi, v, (hi - lo) / 2)
            return res
        if o.kind == 4:  # depthwise 3x3 + bias + relu
            self._check_exact([(x, self.w[o.layer], L.stride)], self.b[o.layer], 3, 1, groups=L.cout)
            s, r = self._acc([(x, self.w[o.layer], L.stride)], pad=1, groups=L.cout)
            lo, hi, v = self._add(s - r, s + r, s, self.b[o.layer].view(1, -1, 1, 1))
            lo, hi, v = self._bf16(*self._relu(lo, hi, v))
            res[o.out] = Out(lo, hi, v, (hi - lo) / 2)
            return res
        if o.kind == 1:  # max-pool 3x3/2 pad 1, affine, relu
            v = F.max_pool2d(x, 3, 2, 1)
            sc, sh = self.aff[o.layer]
            lo, hi, v = self._bf16(*self._relu(*self._affine(v, v, v, sc, sh)))
            res[o.out] = Out(lo, hi, v, (hi - lo) / 2)
            return res
        # conv (kind 2) and the first conv of a back-to-back pair (kind 6)
        if x.shape[1] != L.cin:  # a channel slice of a wider tensor
            x = x[:, o.x_coff:o.x_coff + L.cin]
        dx = None
        if o.in_affine >= 0:
            x, dx = self._operand(x, *self.aff[o.in_affine])
        w, bias = self.w[o.layer], self.b[o.layer]
        if o.layer_n2 >= 0:  # sibling conv on the same input fused along N: its output channels follow
            w = torch.cat([w, self.w[o.layer_n2]], 0)
            bias = torch.cat([bias, self.b[o.layer_n2]], 0)
        segs = [(x, w, L.stride)]
        if o.layer2 >= 0:  # 1x1 shortcut conv as a second K segment of the same GEMM; the two biases are summed in f32
            L2 = g.layers[o.layer2]
            segs.append((tens[o.in2], self.w[o.layer2], L2.stride))
            bias = bias + self.b[o.layer2]
            if self.exact:
                assert torch.equal(bias.float().double(), bias)
        self._check_exact(segs, bias, L.kh, L.pad)
        s, r = self._acc(segs, pad=L.pad)
        if dx is not None and self.radius:   # operands whose own rounding is undecided
            r = r + F.conv2d(dx, w.abs(), None, stride=L.stride, padding=L.pad)
        bw = U * bias.abs().view(1, -1, 1, 1) if (self.radius and o.layer2 >= 0) else 0.0
        lo, hi, v = self._add(s - r - bw, s + r + bw, s, bias.view(1, -1, 1, 1))
        rt = None
        if o.res >= 0:
            rt = tens[o.res]
            if o.res_up2:
                rt = F.interpolate(rt, scale_factor=2, mode="nearest")
            if not o.res_post:
                lo, hi, v = self._add(lo, hi, v, rt)
        if o.out >= 0:
            ylo, yhi, yv = self._relu(lo, hi, v) if o.relu else (lo, hi, v)
            if rt is not None and o.res_post:
                ylo, yhi, yv = self._add(ylo, yhi, yv, rt)
            ylo, yhi, yv = self._bf16(ylo, yhi, yv)
            nout = min(yv.shape[1], o.n_valid)
            dst = np.array([o.y_coff + n + (o.y_split_add if n >= o.y_split else 0) for n in range(nout)])
            res[o.out] = Out(ylo[:, :nout], yhi[:, :nout], yv[:, :nout], (yhi - ylo)[:, :nout] / 2, dst=dst)
        if o.out2 >= 0:
            sc, sh = self.aff[o.layer]
            a = self._bf16(*self._relu(*self._affine(lo, hi, v, sc, sh)))
            res[o.out2] = Out(*a, (a[1] - a[0]) / 2)
        if o.outf >= 0:
            res[o.outf] = Out(lo, hi, v, torch.maximum(v - lo, hi - v), is_f32=True, softmax=bool(o.head_softmax))
        return res

    def b2b_second(self, i, first, chunk=0):
        """out_b of back-to-back op i: relu(conv1x1(a) + bias), a = bf16(relu(affine(raw))) of the device's stored raw output
        (or its stored activated output when the op has no raw one).  first: NCHW f64 of that stored tensor.  chunk: as run_op."""
        if chunk <= 0 or chunk >= first.shape[0]:
            return self._b2b_second(i, first)
        return _cat([self._b2b_second(i, first[k:k + chunk]) for k in range(0, first.shape[0], chunk)])

    def _b2b_second(self, i, first):
        o = self.g.ops[i]
        if o.out >= 0:
            a, dx = self._operand(first, *self.aff[o.layer])
        else:
            a, dx = first, None
        w, bias = self.w[o.layer_b], self.b[o.layer_b]
        self._check_exact([(a, w, 1)], bias, 1, 0)
        s, r = self._acc([(a, w, 1)])
        if dx is not None and self.radius:
            r = r + F.conv2d(dx, w.abs())
        lo, hi, v = self._add(s - r, s + r, s, bias.view(1, -1, 1, 1))
        lo, hi, v = self._bf16(*self._relu(lo, hi, v))
        return Out(lo, hi, v, (hi - lo) / 2)

    def _check_exact(self, segs, bias, kh, pad, groups=1):
        """dyadic set: sum |a b| + |bias| < 2^24 units of the products' grid, so any f32 summation order is exact"""
        if not self.exact:
            return
        e = max([grid_exponent(x) + grid_exponent(w) for x, w, _ in segs] + [grid_exponent(bias)])
        tot = None
        p = pad
        for x, w, st in segs:
            c = F.conv2d(x.abs(), w.abs(), None, stride=st, padding=p, groups=groups)
            tot = c if tot is None else tot + c
            p = 0
        big = float(tot.max()) + float(bias.abs().max())
        assert big * 2.0 ** e < 2.0 ** 24, "dyadic set: sum |a b| = %g on the 2^-%d grid is not exact in f32" % (big, e)


# ---- verdicts ----
def check_bf16(got, out):
    """got: NCHW f64 of the stored bf16 values (the op's channels).  Returns (bad mask, undecided mask)."""
    ok = (got >= out.lo) & (got <= out.hi)   # NaN (an element never written) compares false
    return ~ok, out.lo != out.hi


def check_f32(got, out):
    """f32 head planes.  Box / landmark channels: |got - v64| <= r + 1 ulp.  Soft-maxed score channels 0..3: within 4 ulp of
    the f64 softmax of the interval.  Returns (bad mask, ratio |got - v64| / r over the un-soft-maxed channels)."""
    ulp = lambda z: torch.ldexp(torch.ones_like(z), (torch.frexp(z.float().double())[1] - 24).to(torch.float64))
    bad = torch.zeros_like(got, dtype=torch.bool)
    c0 = 4 if out.softmax else 0
    err = (got[:, c0:] - out.v[:, c0:]).abs()
    bad[:, c0:] = ~(err <= out.rad[:, c0:] + ulp(out.v[:, c0:]))
    rr = out.rad[:, c0:]
    ratio = float((err[rr > 0] / rr[rr > 0]).max()) if bool((rr > 0).any()) else 0.0
    if out.softmax:  # channels 0,1 = bg(a), 2,3 = fg(a): p_fg = 1 / (1 + exp(bg - fg)), monotone in d = bg - fg
        for a in range(2):
            dlo = out.lo[:, a] - out.hi[:, 2 + a]
            dhi = out.hi[:, a] - out.lo[:, 2 + a]
            for c, lo_, hi_ in ((2 + a, torch.sigmoid(-dhi), torch.sigmoid(-dlo)), (a, torch.sigmoid(dlo), torch.sigmoid(dhi))):
                g = got[:, c]
                bad[:, c] = ~((g >= lo_ - 4 * ulp(lo_)) & (g <= hi_ + 4 * ulp(hi_)))
    return bad, ratio
