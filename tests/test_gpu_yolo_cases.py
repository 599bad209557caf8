"""The detector's kernels on the crafted networks of tests/yolo_cases.py, element by element.

One forward pass per (list, batch, mode); every convolution's input and output is downloaded for every image of the batch and compared
with a float64 evaluation of THAT layer on the tensor the GPU itself fed it, under the derived elementwise bound of yolo_cases.py (its
docstring: the derivation; tests/test_yolo_cases.py: the bound rejects every mutant on every one of these layers, and the lists reach every
kernel instantiation the planner can choose).  Then what moves data without arithmetic is compared bit for bit (routes, both ways of
building them), the heads' decode and the post-processing against the numpy restatement on the GPU's own tensors, image by image, and the
lists the forward cannot run against creation itself.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import yolo_cases as yc

pytestmark = pytest.mark.gpu
CHUNK = 8                   # images per float64 evaluation
ERRORS = {}                 # kernel instantiation -> (worst error / bound, where)


@contextlib.contextmanager
def _stop_on_a_device_error(pkg):
    """A HIP error ends the session: nothing more is started on a device that has faulted."""
    try:
        yield
    except pkg.frontend.SdError as e:
        if e.code == pkg.frontend.SD_ERR_HIP:
            pytest.exit("HIP error, no further GPU work in this session: %s" % e, returncode=3)
        raise


def _layers(pkg, c):
    assert pkg.yolo.LAYER_DTYPE == yc.LAYER_DTYPE and (pkg.yolo.CONV, pkg.yolo.YOLO) == (yc.CONV, yc.YOLO)
    return np.ascontiguousarray(c.layers.astype(pkg.yolo.LAYER_DTYPE))


@pytest.fixture(scope="module", params=[(n, b, m) for (n, b) in yc.RUNS for m in yc.MODES], ids=lambda p: "%s-n%d-%s" % p)
def run(request, gpu, pkg):
    """One batch pass and one batch-1 pass per image, everything the tests read downloaded once."""
    import torch
    name, batch, mode = request.param
    c = yc.CASE[name]
    frames = c.frames(batch)
    W, H = c.net_w, c.net_h
    dev = torch.from_numpy(frames).cuda()
    pitch = W * H * 3
    d = pkg.yolo.Detector(_layers(pkg, c), c.anchors, W, H, max_batch=batch, precision=mode)
    try:
        with _stop_on_a_device_error(pkg):
            payload, _ = c.weights()
            assert d.weight_count() == len(payload)
            d.load_weights(payload)
            d.forward_device(dev.data_ptr(), W, H, W * 3, pitch, batch, 0.5)
            stored = [i for i, l in enumerate(c.layers) if l["type"] != yc.UPSAMPLE]
            outs = {i: np.stack([d.layer_output(i, image=k) for k in range(batch)]) for i in stored}
            padded = {i: np.stack([d.layer_stored(i, image=k) for k in range(batch)]) for i in c.convs if c.layers[i]["filters"] % 32}
            host = [d.boxes(k, W, H, 0.5, 0.4) for k in range(batch)]
            device = d.boxes_batch(batch, W, H, 0.5, 0.4)
            single = []
            for k in range(batch):
                d.forward_device(dev.data_ptr() + k * pitch, W, H, W * 3, pitch, 1, 0.5)
                single.append(dict(rows=d.region_rows(), heads={h: d.layer_output(h - 1) for h in c.heads}, boxes=d.boxes(0, W, H, 0.5, 0.4),
                                   device=d.boxes_batch(1, W, H, 0.5, 0.4)[0]))
    finally:
        d.close()
    return dict(case=c, batch=batch, mode=mode, frames=frames, outs=outs, padded=padded, host=host, device=device, single=single, plan=yc.plan(c, mode, batch))


def _write_errors():
    lines = ["worst |got - ref| / bound per kernel instantiation over the crafted networks (tests/test_gpu_yolo_cases.py)",
             "%-28s %9s  %s" % ("kernel", "err/bound", "list, batch, mode, layer, (image, y, x, channel)")]
    lines += ["%-28s %9.4f  %s" % (k, ERRORS[k][0], ERRORS[k][1]) for k in sorted(ERRORS)]
    text = "\n".join(lines) + "\n"
    out = os.environ.get("SD_TEST_REPORT_DIR")          # where a run keeps its tables (profiles/yolo_crafted_errors.txt is a copy of this one)
    if out and os.path.isdir(out):
        open(os.path.join(out, "yolo_crafted_errors.txt"), "w").write(text)
    return text


def test_every_convolution_within_the_elementwise_bound(run):
    c, mode, batch, outs = run["case"], run["mode"], run["batch"], run["outs"]
    act = np.float16 if mode == "f16" else np.float32
    blob = c.blobs(run["frames"], mode)
    failures = []
    for i in c.convs:
        kernel = run["plan"]["convs"][i][0]
        got_all = outs[i]
        assert got_all.dtype == act and np.isfinite(got_all).all(), (c.name, mode, i)
        r = c.residual_of(i)
        worst = (0.0, None)
        for k0 in range(0, batch, CHUNK):
            sl = slice(k0, min(k0 + CHUNK, batch))
            ev = c.evaluate(i, blob[sl] if i == 0 else outs[i - 1][sl], mode, None if r is None else outs[r][sl])
            got = got_all[sl].astype(np.float64)
            assert got.shape == ev.out.shape, (c.name, mode, i, got.shape, ev.out.shape)
            ratio = np.abs(got - ev.out) / ev.bound()
            at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            if ratio[at] >= worst[0]:
                worst = (float(ratio[at]), (k0 + int(at[0]),) + tuple(int(v) for v in at[1:]), float(got[at]), float(ev.out[at]))
        where = "%s n=%d %s layer %d %s" % (c.name, batch, mode, i, worst[1])
        if kernel not in ERRORS or worst[0] > ERRORS[kernel][0]:
            ERRORS[kernel] = (worst[0], where)
        if not worst[0] <= 1.0:
            failures.append("%s on %s: error / bound = %.3g (got %.9g, reference %.9g)" % (where, kernel, worst[0], worst[2], worst[3]))
    print(_write_errors())
    assert not failures, "\n".join(failures)


def test_the_next_layer_reads_exactly_the_filters_of_a_convolution(run):
    """A [shortcut], 1-input [route] or [yolo] behind a convolution reads the convolution's own storage: the same bits, `filters` channels --
    through the stored stride of 256 for a 255-channel head, through the route's stride for a tensor written in place -- and the 256th stored
    channel of a head is still zero."""
    c, outs = run["case"], run["outs"]
    for i, l in enumerate(c.layers):
        t = int(l["type"])
        src = i - 1 if t in (yc.SHORTCUT, yc.YOLO) else c.resolve(i, l["from"][0]) if t == yc.ROUTE and l["nfrom"] == 1 else None
        if src is None:
            continue
        assert outs[i].shape == outs[src].shape and outs[i].tobytes() == outs[src].tobytes(), (c.name, run["mode"], i)
    for i in c.convs:
        assert outs[i].shape[-1] == int(c.layers[i]["filters"])
    # the stored padding of a 255-channel tensor stays zero through the batch pass (the head's kernels write 255 of the 256 stored channels)
    assert sorted(run["padded"]) == [i for i in c.convs if c.layers[i]["filters"] == 255]
    for i, p in run["padded"].items():
        assert p.shape == outs[i].shape[:-1] + (256,) and p[..., :255].tobytes() == outs[i].tobytes(), (c.name, run["mode"], i)
        assert not p[..., 255].any(), "%s %s layer %d: the padding channel of the 255-channel tensor was written" % (c.name, run["mode"], i)


def test_route_outputs_are_their_inputs_bit_for_bit(run):
    """A 2-input [route] holds its first input up-sampled by 2 and its second input, bit for bit: written in place by the producer in the
    f32-class modes (partial, odd), copied whole where a second route reads the skip tensor (dense-route) and in the f16 mode."""
    c, mode, outs = run["case"], run["mode"], run["outs"]
    for i, l in enumerate(c.layers):
        if l["type"] != yc.ROUTE or l["nfrom"] != 2:
            continue
        a, b = outs[c.resolve(i, l["from"][0]) - 1], outs[c.resolve(i, l["from"][1])]
        want = np.concatenate([yc.upsample2(a), b], -1)
        assert np.abs(want).max() > 0
        assert outs[i].shape == want.shape and outs[i].tobytes() == want.tobytes(), (c.name, mode, i, run["plan"]["routes"][i])
        assert run["plan"]["routes"][i] == ("copy" if mode == "f16" or c.name == "dense-route" else "inplace")


def _same_boxes(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_heads_decode_and_boxes_image_by_image(run, pkg):
    """Given the GPU's own head tensors: region_rows() of a batch-1 pass equals the numpy region decode per head, concatenated in head order
    (tolerance: test_gpu_yolo.py's); boxes() and boxes_batch() of EVERY image of the batch pass equal yolo_oracle.postprocess of that image's
    rows exactly -- the rows of its batch-1 pass, whose boxes are the same again.  Two heads, one head, no head; 86 images per decode
    workgroup at batch 96 of the 32 x 32 list."""
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    c, mode, batch = run["case"], run["mode"], run["batch"]
    W, H = c.net_w, c.net_h
    n_rows = sum(run["outs"][h].shape[1] * run["outs"][h].shape[2] * 3 for h in c.heads)
    total = 0
    for k in range(batch):
        s = run["single"][k]
        assert s["rows"].shape == (n_rows, 85)
        if c.heads:
            want = np.concatenate([yo.region_decode(s["heads"][h], list(c.layers[h]["mask"]), c.anchors, W, H) for h in c.heads])
            assert np.allclose(s["rows"], want, rtol=2e-6, atol=1e-7), (c.name, mode, k)
        eb, ec, ef = yo.postprocess(s["rows"], W, H, 0.5, 0.4)
        exp = (eb, ec, ef)
        total += len(eb)
        for what, got in (("boxes() of the batch pass", run["host"][k]), ("boxes_batch() of the batch pass", run["device"][k]),
                          ("boxes() of the batch-1 pass", s["boxes"]), ("boxes_batch() of the batch-1 pass", s["device"])):
            assert _same_boxes(got, exp), "%s n=%d %s image %d: %s differ from postprocess of the image's rows (%d boxes against %d)" % (
                c.name, batch, mode, k, what, len(got[0]), len(eb))
    assert (total > 0) == bool(c.heads), (c.name, mode, total)


@pytest.mark.parametrize("mode", yc.MODES)
def test_batch_slot_does_not_change_a_convolutions_bits(gpu, pkg, mode):
    """`odd`: one image at slots 0 and 4 of a batch of five, and alone: every convolution's output bit for bit the same, in every mode."""
    import torch
    c = yc.CASE["odd"]
    f = c.frames(4)
    frames = np.stack([f[0], f[1], f[2], f[3], f[0]])
    W, H = c.net_w, c.net_h
    dev = torch.from_numpy(frames).cuda()
    d = pkg.yolo.Detector(_layers(pkg, c), c.anchors, W, H, max_batch=5, precision=mode)
    try:
        with _stop_on_a_device_error(pkg):
            d.load_weights(c.weights()[0])
            d.forward_device(dev.data_ptr(), W, H, W * 3, W * H * 3, 5, 0.5)
            five = {(i, k): d.layer_output(i, image=k) for i in c.convs for k in (0, 4)}
            d.forward_device(dev.data_ptr(), W, H, W * 3, W * H * 3, 1, 0.5)
            one = {i: d.layer_output(i, image=0) for i in c.convs}
    finally:
        d.close()
    moved = [(i, "slots 0 and 4") for i in c.convs if five[(i, 0)].tobytes() != five[(i, 4)].tobytes()]
    moved += [(i, "a batch of one and of five") for i in c.convs if one[i].tobytes() != five[(i, 0)].tobytes()]
    kernels = {b: yc.plan(c, mode, b)["convs"] for b in (1, 5)}
    assert not moved, "%s: convolution outputs differ between %s" % (mode, ["layer %d (%s / %s): %s" % (i, kernels[1][i][0], kernels[5][i][0], w) for i, w in moved])


@pytest.mark.parametrize("mode", yc.MODES)
@pytest.mark.parametrize("what", list(yc.REFUSED))
def test_lists_the_forward_cannot_run_are_refused_at_creation(gpu, pkg, what, mode):
    """sd_yolo_create_prec answers SD_ERR_UNSUPPORTED or SD_ERR_INVALID with a message and creates no detector: the forward pass is never
    asked to run such a list (an unfused [shortcut] used to be refused in the middle of it, behind the launches of the layers before)."""
    fe = pkg.frontend
    ls, w, h = yc.REFUSED[what]
    layers = np.ascontiguousarray(yc.layer_array(ls).astype(pkg.yolo.LAYER_DTYPE))
    anchors = np.ascontiguousarray(yc.ANCHORS)
    L = fe.lib()
    vp, i = C.c_void_p, C.c_int
    L.sd_yolo_create_prec.argtypes = [C.POINTER(vp), vp, i, vp, i, i, i, i, i]
    handle = C.c_void_p(0xdead)
    rc = L.sd_yolo_create_prec(C.byref(handle), fe._p(layers), len(layers), fe._p(anchors), 80, w, h, 1, yc.PRECS[mode])
    assert rc in (fe.SD_ERR_UNSUPPORTED, fe.SD_ERR_INVALID), (what, rc)
    assert not handle.value, "no detector may be created"
    assert (L.sd_last_error() or b"").decode().strip(), "the refusal carries a message"
    assert yc.plan_many([(ls, w, h, mode, 1)])[0]["refused"][0] == rc
