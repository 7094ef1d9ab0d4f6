"""GPU tests of the convolution engine and the whole network.

(1) every op of the graph in isolation (seeded bf16 inputs written through the debug hooks) against
    torch-CPU f32 on the same bf16-rounded inputs and weights: tolerance = 1 bf16 ulp of the result
    (2^-7 relative) plus the f32 accumulation-order noise;
(2) the whole forward pass against the torch emulation that rounds to bf16 at the same points;
(3) the fused pipeline (rfd_detect_batch) against the oracle's decode/NMS of the SAME head tensors:
    identical kept-anchor sequences, coordinates within 1e-4.
CNN parity to the reference itself is unpinned: the model file is not in the reference."""
import numpy as np
import pytest
import torch

import helpers
import torch_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["r50", "mnet025"])
def net(rfd, request):
    """RetinaFace-R50 (BASELINE configs[2]) and RetinaFace-MobileNet-0.25 (configs[1]), same tests."""
    bb = rfd.BACKBONE_R50 if request.param == "r50" else rfd.BACKBONE_MNET025
    det = rfd.RetinaFaceDetection(image_size=(640, 640), max_batch_size=2, max_det=2048, backbone=bb)
    det.init_synthetic_weights(1234)
    g = rfd.Graph(bb, 640, 640)
    ref = torch_ref.TorchRef(g, det)
    yield det, g, ref
    det.close()


def _rand_act(rng, n, td, relu_like=True):
    x = rng.normal(0, 1, size=(n, td.channels_logical, td.height, td.width)).astype(np.float32)
    if relu_like:
        x = np.maximum(x, 0)
    return torch.from_numpy(helpers.bf16_round(x))


def _check_close(got, want, what):
    got, want = got.numpy(), want.numpy()
    scale = float(np.sqrt(np.mean(want.astype(np.float64) ** 2))) + 1e-6
    err = np.abs(got - want)
    tol = 2.0 ** -7 * np.abs(want) + 3e-3 * scale
    bad = err > tol
    assert not bad.any(), "%s: %d / %d outside tolerance, max err %.4g (rms %.3g)" % (
        what, int(bad.sum()), bad.size, float(err.max()), scale)
    return float(np.mean(got == want))


@pytest.mark.parametrize("tile", [0, 1, 2, 6, 17])
def test_every_op_in_isolation(rfd, net, tile):
    """tile 17: the wave-specialised ring (kernels_ring.hip) wherever the layer shape allows; tile 0: the production heuristic (merged-kx 3x3 kernel, asymmetric rings, persistent kernels where the problem is
    large enough); tile 6: the same with the persistent kernels (pw_stream, conv3x3_c64) forced at this small batch; tile 1: every conv on the generic 128-row, 2-slot tiles; tile 2: the 256x128, 3-slot-ring tile wherever
    Cout % 128 == 0 (the heuristic picks between them by grid size at run time)."""
    det, g, ref = net
    det.debug_set_conv_tile(tile)
    rng = np.random.default_rng(99)
    n = 2
    exact = []
    per_op = {}
    for i, o in enumerate(g.ops):
        if tile == 2 and (o.kind != 2 or g.layers[o.layer].cout % 128 or o.layer_n2 >= 0):  # (kind 6 has its own kernel)
            continue
        tens = {}
        tin = g.tensors[o.in_]
        if o.kind in (0, 3, 5):
            x = rng.integers(0, 256, size=(n, 4, tin.height, tin.width)).astype(np.float32)
            x[:, 3] = 0
            tens[o.in_] = torch.from_numpy(x)
        else:
            tens[o.in_] = _rand_act(rng, n, tin, relu_like=o.in_affine < 0)
        det.debug_write(o.in_, torch_ref.nchw_to_dev(tens[o.in_], channels=g.tensors[o.in_].channels))
        if o.in2 >= 0:
            tens[o.in2] = _rand_act(rng, n, g.tensors[o.in2])
            det.debug_write(o.in2, torch_ref.nchw_to_dev(tens[o.in2], channels=g.tensors[o.in2].channels))
        if o.res >= 0:
            tens[o.res] = _rand_act(rng, n, g.tensors[o.res], relu_like=False)
            det.debug_write(o.res, torch_ref.nchw_to_dev(tens[o.res], channels=g.tensors[o.res].channels))
        if o.out >= 0 and o.out != o.in_ and g.tensors[o.out].channels_logical != g.layers[o.layer].cout:
            # SSH concat slice: pre-fill the destination so untouched channels can be checked too
            tens[o.out] = _rand_act(rng, n, g.tensors[o.out])
            det.debug_write(o.out, torch_ref.nchw_to_dev(tens[o.out], channels=g.tensors[o.out].channels))
        det.debug_run(n, i, i)
        with torch.no_grad():
            ref.run_op(i, tens)
        for t in (o.out, o.out2, o.outf, o.out_b):
            if t < 0:
                continue
            td = g.tensors[t]
            got = torch_ref.dev_to_nchw(det.debug_read(t, n, td), bool(td.is_f32), td.channels_logical)
            exact.append(_check_close(got, tens[t], "op %d (%s) tensor %d" % (i, g.layers[o.layer].name.decode(), t)))
            if not td.is_f32:   # f32 heads: torch's own f32 order differs in the last bits (checked against f64 in test_conv_exact_gpu)
                per_op.setdefault(i, []).append(exact[-1])
    det.debug_set_conv_tile(0)
    assert np.mean(exact) > 0.97  # nearly every bf16 output is bit-identical to the torch result
    worst = min(per_op, key=lambda i: min(per_op[i]))
    assert min(per_op[worst]) > 0.97, "op %d: only %.4f of the bf16 outputs equal the torch result" % (worst, min(per_op[worst]))


def test_batch_tail_rows(rfd, net):
    """B = 1 makes M = 400 / 1600 at the deep stages: not a multiple of the 128-row tile."""
    det, g, ref = net
    rng = np.random.default_rng(5)
    for i, o in enumerate(g.ops):
        L = g.layers[o.layer]
        if o.kind != 2 or g.tensors[o.in_].height > 40:
            continue
        tens = {o.in_: _rand_act(rng, 1, g.tensors[o.in_])}
        det.debug_write(o.in_, torch_ref.nchw_to_dev(tens[o.in_], channels=g.tensors[o.in_].channels))
        if o.in2 >= 0:
            tens[o.in2] = _rand_act(rng, 1, g.tensors[o.in2])
            det.debug_write(o.in2, torch_ref.nchw_to_dev(tens[o.in2], channels=g.tensors[o.in2].channels))
        if o.res >= 0:
            tens[o.res] = _rand_act(rng, 1, g.tensors[o.res], relu_like=False)
            det.debug_write(o.res, torch_ref.nchw_to_dev(tens[o.res], channels=g.tensors[o.res].channels))
        if o.out >= 0 and o.out != o.in_ and g.tensors[o.out].channels_logical != L.cout:
            tens[o.out] = _rand_act(rng, 1, g.tensors[o.out])
            det.debug_write(o.out, torch_ref.nchw_to_dev(tens[o.out], channels=g.tensors[o.out].channels))
        det.debug_run(1, i, i)
        with torch.no_grad():
            ref.run_op(i, tens)
        for t in (o.out, o.out2, o.outf):
            if t >= 0:
                td = g.tensors[t]
                _check_close(torch_ref.dev_to_nchw(det.debug_read(t, 1, td), bool(td.is_f32), td.channels_logical), tens[t], "op %d" % i)


def _frames():
    return [helpers.make_image(101, 720, 1000), helpers.make_image(102, 1080, 1920)]


def test_forward_matches_torch_emulation(rfd, oracle, net):
    det, g, ref = net
    frames = _frames()
    tensor = np.stack([oracle.preprocess(f, 640, 640)[1] for f in frames])
    heads = det.forward(tensor)
    x4 = torch.cat([torch.from_numpy(tensor), torch.zeros(2, 1, 640, 640)], 1)
    want = ref.heads(ref.forward(x4))
    for k, (a, b) in enumerate(zip(heads, want)):
        assert a.shape == b.shape
        err = np.abs(a - b)
        rms = float(np.sqrt(np.mean(b.astype(np.float64) ** 2)))
        # bf16 activations: 1-ulp flips (0.4 %) propagate through ~55 layers; the two implementations
        # must still agree to a few percent of the signal everywhere and far better on average
        assert float(np.mean(err)) < 0.01 * rms + 1e-4, (k, float(np.mean(err)), rms)
        assert float(err.max()) < 0.15 * rms + 2e-2, (k, float(err.max()), rms)
    for l in range(3):  # softmax pairs sum to one
        cls = heads[3 * l]
        np.testing.assert_allclose(cls[:, 0:2] + cls[:, 2:4], 1.0, atol=1e-5)


def test_fused_pipeline_matches_oracle_on_same_heads(rfd, oracle, net):
    det, g, ref = net
    frames = _frames()
    pre = [oracle.preprocess(f, 640, 640) for f in frames]
    tensor = np.stack([p[1] for p in pre])
    heads = det.forward(tensor)
    # pick the threshold so that ~1 % of the anchors are candidates with these random weights
    fg = np.concatenate([heads[3 * l][:, 2:4].reshape(2, -1) for l in range(3)], 1)
    thr = float(np.quantile(fg, 0.99))
    det.set_thresholds(thr, 0.45)
    got = det.call_batch(frames)
    st = det.stats()
    assert st["candidates"] >= 200
    for b in range(2):
        odet, olmk, ogidx, ncand = oracle.decode_nms([h[b] for h in heads], 640, 640, np.float32(thr), 0.45,
                                                     det_scale=float(pre[b][2]))
        gdet, glmk = got[b]
        assert len(gdet) == len(odet) == det.last_total[b] and len(odet) >= 1
        assert np.array_equal(gdet[:, 4], odet[:, 4])                       # same anchors, same order
        assert np.array_equal(gdet, odet[:, :5]) and np.array_equal(glmk, olmk)  # the post-network path is bit-identical
    # the single-image entry point (`call`) returns the same rows as the batch
    d0, k0 = det.call(frames[0])
    assert np.array_equal(d0, got[0][0]) and np.array_equal(k0, got[0][1])
    det.set_thresholds(0.7, 0.45)


def test_macs_match_graph_description(rfd, net):
    det, g, ref = net
    want = {"r50": 44.2646528e9, "mnet025": 0.9811456e9}[
        "r50" if g.num_layers == 76 else "mnet025"]
    assert abs(g.macs - want) < 1e3


def test_uninitialised_weights_are_an_error(rfd):
    d = rfd.RetinaFaceDetection(max_batch_size=1)
    with pytest.raises(rfd.RfdError) as e:
        d.call(helpers.make_image(1, 64, 64))
    assert e.value.status == rfd.RFD_ERR_STATE
    d.close()


def test_weight_file_roundtrip(rfd, tmp_path):
    """rfd_save_weights -> rfd_load_weights into a fresh context reproduces the detections bit for bit;
    a file of the other backbone or a truncated file is refused."""
    a = rfd.RetinaFaceDetection(max_batch_size=1, max_det=256, backbone=rfd.BACKBONE_MNET025, confidence_threshold=0.3)
    a.init_synthetic_weights(77)
    frame = helpers.make_image(5, 480, 640)
    want = a.call(frame)
    path = str(tmp_path / "mnet.rfdw")
    a.save_weights(path)
    b = rfd.RetinaFaceDetection(max_batch_size=1, max_det=256, backbone=rfd.BACKBONE_MNET025, confidence_threshold=0.3)
    b.load_weights(path)
    got = b.call(frame)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and len(want[0]) > 0
    c = rfd.RetinaFaceDetection(max_batch_size=1, backbone=rfd.BACKBONE_R50)
    with pytest.raises(rfd.RfdError) as e:
        c.load_weights(path)
    assert e.value.status == rfd.RFD_ERR_INVALID_ARG
    data = open(path, "rb").read()
    open(path, "wb").write(data[: len(data) // 2])
    with pytest.raises(rfd.RfdError) as e:
        b.load_weights(path)
    assert e.value.status == rfd.RFD_ERR_IO
    with pytest.raises(rfd.RfdError) as e:
        b.load_weights(str(tmp_path / "missing.rfdw"))
    assert e.value.status == rfd.RFD_ERR_IO
    for d in (a, b, c):
        d.close()
