"""Every conv-path kernel the launcher can pick, on every op, against the f64 reference of tests/exact_ref.py.

plan() asks the library which kernel(s) each op would run under every force_tile value (nothing is launched) and keeps one
case per distinct kernel list.  Each case runs once on two input sets:
- dyadic: weights k 2^-6 (|k| <= 8), biases on 2^-10, power-of-two affine scales, shifts on 2^-4, activations j 2^-4, pixels
  0..255.  Every f32 sum and epilogue step is then exact in any order, so every bf16 output must equal RNE(v64) bit for bit;
- random: the synthetic weights and the ReLU'd-normal activations of test_network_gpu.py.  Every decided element must match,
  every undecided one must lie in its interval, and the undecided share of an op stays <= 10 % (the bound is not vacuous).
Outputs are poisoned with NaN before the launch: every element the op writes must be overwritten, every other byte kept.

test_plan_covers_every_kernel_instantiation: a conv-path kernel is in the shipped code objects if and only if this sweep runs it
(no exceptions list: a kernel that only an environment variable, or nothing, could select does not ship)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import exact_ref
import torch_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "rs-face-detection_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"

# (backbone, image w, image h, images per chain, ops: None = all; "large": the stem and the 1x1 convs on maps <= 40 rows, the
#  layers whose kernel choice changes between 5 images and a production chain of 16)
GEOMETRIES = [
    ("r50", 640, 640, 1, None), ("r50", 640, 640, 2, None), ("r50", 768, 480, 3, None), ("r50", 480, 352, 5, None),
    ("r50", 96, 64, 3, None), ("r50", 32, 32, 4, None),
    ("r50", 640, 640, 4, None),     # 25 600-pixel stride-8 maps: pw_gemm's 128 x 256 items (N = 256, >= 150 of them)
    ("r50", 640, 640, 16, "large"),  # >= 2048 stem tiles: the persistent stem kernel (alone and with conv1 fused); stage 3's 1x1s
    ("mnet025", 640, 640, 1, None), ("mnet025", 640, 640, 2, None), ("mnet025", 768, 480, 3, None),
    ("mnet025", 480, 352, 5, None), ("mnet025", 96, 64, 3, None), ("mnet025", 32, 32, 4, None),
]
TILES = range(20)  # every force_tile value launch_conv knows (0 = the production heuristic)

NAN_BF16 = 0x7FC0
NAN_F32 = 0x7FC00000


def _bb(rfd, name):
    return rfd.BACKBONE_R50 if name == "r50" else rfd.BACKBONE_MNET025


def plan(det, g, n, ops=None):
    """[(op, kernel names, force_tile, last op of the run)]: one case per distinct kernel list of every op.  The stem and the
    conv behind it run as ONE launch when the library fuses them (reported as "(fused into ...)" for the conv): that case runs
    both ops and checks both outputs."""
    cases = []
    idx = range(len(g.ops)) if ops is None else [i for i, o in enumerate(g.ops) if o.kind == 3 or (
        o.kind in (2, 6) and g.layers[o.layer].kh == 1 and g.tensors[o.in_].height <= 40)]
    try:
        for i in idx:
            seen = set()
            for tile in TILES:
                det.debug_set_conv_tile(tile)
                names = tuple(det.debug_op_kernels(n, i, co_running=False))
                if names[0].startswith("(fused into") or names in seen:
                    continue
                seen.add(names)
                last = i
                if g.ops[i].kind == 3 and i + 1 < len(g.ops):
                    if det.debug_op_kernels(n, i + 1, co_running=False)[0].startswith("(fused into"):
                        last = i + 1
                cases.append((i, names, tile, last))
    finally:
        det.debug_set_conv_tile(0)
    return cases


def _dyadic_weights(det, g, rng):
    """Ops whose second conv reads the op's own stored output (the stem + fused conv1, the back-to-back pairs) keep that
    operand on a coarse grid: the stem's bias on 2^-6, affine scales +-1 on the stored output, small second-conv weights.
    ExactRef(exact=True) asserts that every sum stays exact in f32."""
    feeds = {o.layer for o in g.ops if o.kind in (3, 6)}
    second = {o.layer_b for o in g.ops if o.kind == 6}
    for i, L in enumerate(g.layers):
        w, b = det.get_layer(i, L)
        k = 2 if i in second else 8
        bias = rng.integers(-64, 65, size=b.shape) * 2.0 ** -6 if L.kind == 3 else rng.integers(-512, 513, size=b.shape) * 2.0 ** -10
        det.set_layer(i, rng.integers(-k, k + 1, size=w.shape) * 2.0 ** -6, bias)
        if L.has_affine:
            s = rng.choice([1.0, -1.0] if i in feeds else [1.0, 0.5, 0.25, -0.5], size=L.cout)
            det.set_affine(i, s, rng.integers(-16, 17, size=L.cout) * 2.0 ** -4)


def _act(rng, n, td, signed, dyadic):
    shape = (n, td.channels_logical, td.height, td.width)
    if dyadic:
        return torch.from_numpy(rng.integers(-15 if signed else 0, 16, size=shape) * 2.0 ** -4)
    x = rng.normal(0, 1, size=shape).astype(np.float32)
    if not signed:
        x = np.maximum(x, 0)
    return torch.from_numpy(x).to(torch.bfloat16).double()


def _inputs(rng, g, o, n, dyadic):
    L = g.layers[o.layer]
    tin = g.tensors[o.in_]
    tens = {}
    if o.kind in (0, 3, 5):
        x = rng.integers(0, 256, size=(n, 4, tin.height, tin.width)).astype(np.float64)
        x[:, 3] = 0
        tens[o.in_] = torch.from_numpy(x)
    else:
        tens[o.in_] = _act(rng, n, tin, o.in_affine >= 0, dyadic)
    if o.in2 >= 0:
        tens[o.in2] = _act(rng, n, g.tensors[o.in2], False, dyadic)
    if o.res >= 0:
        tens[o.res] = _act(rng, n, g.tensors[o.res], True, dyadic)
    if o.out >= 0 and o.out != o.in_ and g.tensors[o.out].channels_logical != L.cout:
        tens[o.out] = _act(rng, n, g.tensors[o.out], False, dyadic)   # SSH concat slice: the untouched channels keep these
    return tens


def _dev(t, td):
    return torch_ref.nchw_to_dev(t.float(), channels=td.channels)


def _to_f64(a, is_f32):
    if is_f32:
        return torch.from_numpy(a.astype(np.float64)).permute(0, 3, 1, 2)
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)).permute(0, 3, 1, 2)


def _first_bad(bad):
    pos = np.argwhere(bad.numpy())
    return [tuple(int(v) for v in p) for p in pos[:3]]


class Sweep:
    """batch_off / co_running: the cases run as a chain of a split pass does (tests/test_production_plan_gpu.py), on images
    [batch_off, batch_off + n) of a workspace of max_batch images, with the kernel choice of a co-running chain.  Every tensor
    then goes to the device as its WHOLE workspace buffer, NaN outside the chain's images, and every byte outside them must come
    back unchanged.  chunk: images per evaluation of the f64 reference (0: all at once)."""

    def __init__(self, det, g, geo, n, batch_off=0, co_running=False, max_batch=None, chunk=0):
        self.det, self.g, self.geo, self.n = det, g, geo, n
        self.batch_off, self.co_running, self.chunk = batch_off, co_running, chunk
        self.chain = max_batch is not None
        assert self.chain or (batch_off == 0 and not co_running)
        assert not self.chain or batch_off + n <= max_batch
        self.pairs = set()
        self._sent, self._poison = {}, {}
        self.fail = []
        self.cases = 0
        self.names = set()
        self.ties = [0, 0]
        self.undecided = 0.0
        self.ratio = 0.0
        self._cache = {}

    def run_set(self, cases, dyadic, seed):
        det, g, n = self.det, self.g, self.n
        ref = exact_ref.ExactRef(g, det)
        ref.radius, ref.exact = not dyadic, dyadic
        tag = "dyadic" if dyadic else "random"
        rng = np.random.default_rng(seed)
        by_op = {}
        for c in cases:
            by_op.setdefault(c[0], []).append(c)
        for i, ocases in by_op.items():
            o = g.ops[i]
            tens = _inputs(rng, g, o, n, dyadic)
            with torch.no_grad():
                want = ref.run_op(i, tens, self.chunk)
            if dyadic:
                for t, w in want.items():
                    if not w.is_f32:
                        d, u = exact_ref.bf16_ties(w.v)
                        self.ties[0] += d
                        self.ties[1] += u
            else:
                und = [float((w.lo != w.hi).double().mean()) for w in want.values() if not w.is_f32]
                if und:
                    self.undecided = max(self.undecided, max(und))
                    if max(und) > 0.10:
                        self.fail.append("op %d: %.1f %% of the outputs undecided: the radius is too wide" % (i, 100 * max(und)))
            self._cache.clear()
            for (_, names, tile, last) in ocases:
                self.cases += 1
                self.names.update(names)
                self.pairs.add((i, tuple(names)))
                self._run_case(ref, i, tens, want, names, tile, last, tag)

    def _run_case(self, ref, i, tens, want, names, tile, last, tag):
        det, g, n = self.det, self.g, self.n
        o = g.ops[i]
        det.debug_set_conv_tile(tile)
        what = "op %d (%s, kind %d) kernel %s (tile %d) at %s n = %d%s, %s set" % (
            i, g.layers[o.layer].name.decode(), o.kind, " + ".join(names), tile, self.geo, n,
            " at image %d%s" % (self.batch_off, ", co-running" if self.co_running else "") if self.chain else "", tag)
        self._sent.clear()
        for t, x in tens.items():
            self._write(t, _dev(x, g.tensors[t]))
        outs = [(t, i) for t in (o.out, o.out2, o.outf, o.out_b) if t >= 0]
        if last > i:
            outs.append((g.ops[last].out, last))
        prior = {}
        for t, _ in outs:
            td = g.tensors[t]
            if t in tens:
                a = _dev(tens[t], td).copy()
            else:
                a = np.zeros((n, td.height, td.width, td.channels), np.float32 if td.is_f32 else np.uint16)
            written = want[t].dst if (t in want and want[t].dst is not None) else np.arange(td.channels_logical)
            if t == o.in_:
                assert not set(written) & set(range(o.x_coff, o.x_coff + g.layers[o.layer].cin)), "in-place op overwrites its input"
            pa = a.view(np.uint32) if td.is_f32 else a
            pa[..., written] = NAN_F32 if td.is_f32 else NAN_BF16
            self._write(t, a)
            prior[t] = (a.copy(), written)
        det.debug_run(n, i, last, self.batch_off, self.co_running)
        det.debug_set_conv_tile(0)
        for t in tens if self.chain else ():
            if t not in prior:   # an operand the op only reads
                a = _dev(tens[t], g.tensors[t])
                if not np.array_equal(self._read(t, what).view(np.uint8), a.view(np.uint8)):
                    self.fail.append("%s tensor %d: the op changed an operand it only reads" % (what, t))
        for t, oi in outs:
            td = g.tensors[t]
            got = self._read(t, what)
            a, written = prior[t]
            keep = np.setdiff1d(np.arange(td.channels), written)
            if not np.array_equal(np.ascontiguousarray(got[..., keep]).view(np.uint8), np.ascontiguousarray(a[..., keep]).view(np.uint8)):
                self.fail.append("%s tensor %d: bytes outside the op's channels changed" % (what, t))
            g64 = _to_f64(got[..., written], td.is_f32)
            if t in want and oi == i:
                w = want[t]
            else:   # read from the device's own stored first output: out_b of a b2b op, or the conv fused into the stem kernel
                src = o.out if (oi == i and o.out >= 0) else (o.out2 if oi == i else g.ops[oi].in_)
                st = g.tensors[src]
                raw = self._read(src, what)
                first = _to_f64(raw[..., :st.channels_logical], False)
                if bool(torch.isnan(first).any()):   # reported with tensor src itself; the reference cannot start from NaN
                    self.fail.append("%s tensor %d: not checked, the stored tensor %d it is computed from holds NaN" % (what, t, src))
                    continue
                key = (t, raw.tobytes())
                if key not in self._cache:
                    with torch.no_grad():
                        self._cache[key] = ref.b2b_second(i, first, self.chunk) if oi == i else ref.run_op(oi, {src: first}, self.chunk)[t]
                w = self._cache[key]
            if td.is_f32:
                bad, ratio = exact_ref.check_f32(g64, w)
                self.ratio = max(self.ratio, ratio)
            else:
                bad, _ = exact_ref.check_bf16(g64, w)
            if bool(bad.any()):
                p = _first_bad(bad)
                b0 = p[0]
                ex = (g64[b0] - w.v[b0]).abs() / max(float(w.rad[b0]), 1e-300)
                self.fail.append("%s tensor %d: %d / %d elements wrong, first at (n, c, y, x) %s: got %r, legal [%r, %r], v64 %r "
                                 "(%.3g r from v64)" % (what, t, int(bad.sum()), bad.numel(), p, float(g64[b0]), float(w.lo[b0]),
                                                        float(w.hi[b0]), float(w.v[b0]), float(ex)))

    def _write(self, t, a):
        """the n images of tensor t; in chain mode inside its whole buffer, NaN bits everywhere else"""
        if not self.chain:
            self.det.debug_write(t, a)
            return
        td = self.g.tensors[t]
        pitch = self.det.debug_buffer_pitch(t)
        assert pitch % 4 == 0 and a.nbytes <= self.n * pitch
        nan, u = (NAN_F32, np.uint32) if td.is_f32 else (NAN_BF16, np.uint16)
        key = (self.det.cfg.max_batch_size * pitch, u)
        if key not in self._poison:
            self._poison[key] = np.full(key[0] // np.dtype(u).itemsize, nan, u)
        buf = self._poison[key].view(np.uint8)
        lo = self.batch_off * pitch
        a = np.ascontiguousarray(a)
        buf[lo:lo + a.nbytes] = a.reshape(-1).view(np.uint8)
        self.det.debug_buffer_write(t, buf)
        buf[lo:lo + a.nbytes].view(u)[:] = nan
        self._sent[t] = (lo, a.shape, a.dtype)

    def _read(self, t, what):
        """the n images of tensor t; in chain mode every byte of its buffer outside them must still hold the NaN bits"""
        td = self.g.tensors[t]
        if not self.chain:
            return self.det.debug_read(t, self.n, td)
        buf = self.det.debug_buffer_read(t)
        lo, shape, dt = self._sent[t]
        hi = lo + int(np.prod(shape)) * np.dtype(dt).itemsize
        nan, u = (NAN_F32, np.uint32) if td.is_f32 else (NAN_BF16, np.uint16)
        for name, part in (("before", buf[:lo]), ("behind", buf[hi:])):
            ok = part.view(u) == nan
            if not bool(ok.all()):
                first = int(np.argmin(ok)) * np.dtype(u).itemsize + (0 if name == "before" else hi)
                self.fail.append("%s tensor %d: %d elements %s the chain's images changed, first at byte %d of the buffer (image pitch %d; "
                                 "the chain holds bytes [%d, %d))" % (what, t, int((~ok).sum()), name, first, len(buf) // self.det.cfg.max_batch_size, lo, hi))
        return buf[lo:hi].view(dt).reshape(shape).copy()


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["%s-%dx%d-n%d%s" % (b, w, h, n, "-" + o if o else "") for b, w, h, n, o in GEOMETRIES])
def test_every_kernel_matches_the_f64_reference(rfd, geom):
    bb, w, h, n, ops = geom
    det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=n, max_det=16, backbone=_bb(rfd, bb))
    try:
        det.init_synthetic_weights(1234)
        g = rfd.Graph(_bb(rfd, bb), w, h)
        cases = plan(det, g, n, ops)
        sw = Sweep(det, g, "%s %dx%d" % (bb, w, h), n)
        sw.run_set(cases, dyadic=False, seed=11)
        _dyadic_weights(det, g, np.random.default_rng(12))
        sw.run_set(cases, dyadic=True, seed=13)
        print("\nexact sweep %s %dx%d n=%d: %d cases, %d kernel names, %d failures, ties %d down / %d up, "
              "max undecided %.2f %%, head |got - v64| / r max %.3f" % (bb, w, h, n, sw.cases // 2, len(sw.names), len(sw.fail),
                                                                        sw.ties[0], sw.ties[1], 100 * sw.undecided, sw.ratio))
        assert not sw.fail, "\n".join(sw.fail[:12]) + ("\n... %d more" % (len(sw.fail) - 12) if len(sw.fail) > 12 else "")
        if ops is None:
            assert min(sw.ties) >= 200 and sum(sw.ties) >= 2000, sw.ties   # the dyadic set must really exercise ties-to-even
        if bb == "r50" and ops is None:
            assert 0 < sw.ratio <= 1.0, sw.ratio
    finally:
        det.close()


def _shipped_kernels(tmp):
    names = set()
    for f in ("kernels_conv", "kernels_ring"):
        obj = os.path.join(BUILD, f + ".o")
        fat, co = os.path.join(tmp, f + ".fat"), os.path.join(tmp, f + ".co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        mangled = re.findall(r"^\s+\.name:\s+(_Z\S+)", txt, re.M)
        filt = os.path.join(LLVM, "llvm-cxxfilt")
        filt = filt if os.path.exists(filt) else "c++filt"
        out = subprocess.run([filt], input="\n".join(mangled), check=True, capture_output=True, text=True).stdout
        for line in out.splitlines():
            s = re.sub(r"^void ", "", line.strip()).replace("rfd::", "")
            names.add(s[:s.rindex("(")] if s.endswith(")") else s)
    names.discard("heads_to_nchw_kernel")   # post-network layout kernel, not a conv path
    return names


def test_plan_covers_every_kernel_instantiation(rfd, tmp_path):
    shipped = _shipped_kernels(str(tmp_path))
    assert len(shipped) == 49, sorted(shipped)   # guards the name extraction: 47 in kernels_conv.o, 2 in kernels_ring.o
    reached = set()
    for bb, w, h, n, ops in GEOMETRIES:
        det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=n, max_det=16, backbone=_bb(rfd, bb))
        try:
            det.init_synthetic_weights(1234)
            g = rfd.Graph(_bb(rfd, bb), w, h)
            for _, names, _, _ in plan(det, g, n, ops):
                reached.update(names)
        finally:
            det.close()
    print("\ncoverage: %d shipped conv-path kernels, %d reached by the sweep" % (len(shipped), len(reached)))
    assert shipped == reached, "reached but not shipped (name format drift?): %s; shipped without an exact-reference check: %s" % (
        sorted(reached - shipped), sorted(shipped - reached))


BATCH_RUNS = {"r50": [(640, 640), (768, 480)], "mnet025": [(640, 640)]}


@pytest.mark.parametrize("bb,w,h", [(b, w, h) for b, gs in BATCH_RUNS.items() for w, h in gs])
def test_heads_do_not_depend_on_the_batch_size(rfd, bb, w, h):
    """one K order per layer whatever kernel runs it, so a frame's 9 head tensors are bit-identical whether it
    runs alone (B = 1), in small split batches, or inside a 32-frame batch (two 16-image chains, persistent kernels, stem+conv1
    fusion).  Every position of the passes of 32 (chains of 16 + 16), 17 (9 + 8) and 8 (4 + 4) images is compared with the B = 1
    run of its frame: the positions in the middle of a chain and on both sides of the cut between the chains included."""
    det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=32, max_det=16, backbone=_bb(rfd, bb))
    try:
        det.init_synthetic_weights(1234)
        rng = np.random.default_rng(21)
        frames = rng.uniform(-1.0, 1.0, size=(32, 3, h, w)).astype(np.float32)
        big = frames.copy()
        big[26:32] = frames[0:6]
        alone_big = [det.forward(big[k:k + 1]) for k in range(32)]   # positions 26..31 repeat frames 0..5: runs of their own
        alone = alone_big[:6]
        for j in range(6):
            for lvl, (a, b) in enumerate(zip(alone_big[26 + j], alone[j])):
                assert np.array_equal(a, b), "%s %dx%d frame %d: two B = 1 runs differ in head tensor %d" % (bb, w, h, j, lvl)
        runs = []
        for bs in (2, 3, 8):
            for s0 in range(0, 6, bs):
                batch = frames[[(s0 + j) % 32 if s0 + j < 6 else 6 + j for j in range(bs)]]
                heads = det.forward(batch)
                runs += [("B=%d" % bs, s0 + j, [x[j:j + 1] for x in heads]) for j in range(bs) if s0 + j < 6]
        heads = det.forward(big)
        runs += [("B=32 pos %d" % j, j, [x[j:j + 1] for x in heads]) for j in range(6)]
        runs += [("B=32 pos %d" % (26 + j), j, [x[26 + j:27 + j] for x in heads]) for j in range(6)]
        for tag, k, hs in runs:
            for lvl, (a, b) in enumerate(zip(hs, alone[k])):
                assert np.array_equal(a, b), "%s %dx%d frame %d, %s: head tensor %d differs from the B = 1 run (%d elements)" % (
                    bb, w, h, k, tag, lvl, int((a != b).sum()))
        for B, hs in ((32, heads), (17, det.forward(big[:17])), (8, det.forward(big[:8]))):
            assert len(det.debug_pass_chains(B)) == 2, "a pass of %d images is expected to run as two chains" % B
            for j in range(B):
                for lvl, (a, b) in enumerate(zip(hs, alone_big[j])):
                    assert np.array_equal(a[j:j + 1], b), "%s %dx%d B=%d (chains %s) position %d: head tensor %d differs from the B = 1 " \
                        "run of that frame (%d elements)" % (bb, w, h, B, det.debug_pass_chains(B), j, lvl, int((a[j:j + 1] != b).sum()))
    finally:
        det.close()
