"""The crafted detector networks of tests/yolo_cases.py, on the CPU: do they reach the kernels they are aimed at (coverage, from
csrc/sd_yolo_plan.h compiled with g++ alone), would the elementwise bound notice a subtly wrong kernel (sharpness: every mutant of the
reference must be REJECTED on every layer it applies to), and is the float64 reference the graph the suite's oracle computes (agreement
with oracle/yolo_oracle.torch_forward in float64).  tests/test_gpu_yolo_cases.py then holds the kernels to that reference."""
import os
import re

import numpy as np
import pytest

import yolo_cases as yc

ROOT = yc.ROOT
UNREACHABLE = {"k_conv3x3_b3<3, 2, 2>", "k_conv3x3_b3<4, 2, 2>"}


def kernel_list():
    """The names of SD_YOLO_KERNELS, read from the header (the X-macro is the only list that names them)."""
    src = open(os.path.join(ROOT, "slam-dynamic_amd", "csrc", "sd_yolo_plan.h")).read()
    body = src[src.index("#define SD_YOLO_KERNELS(X)"):src.index("enum SdYoloKernel")]
    names = re.findall(r"X\(\w+, \d+, (.+?)\)(?: \\)?\n", body)
    assert len(names) == 23, names
    return names


@pytest.fixture(scope="module")
def planned():
    """{(list, batch, mode): plan record} for every run of the GPU tests."""
    keys = [(name, b, m) for (name, b) in yc.RUNS for m in yc.MODES]
    recs = yc.plan_many([(yc.CASE[n].layers, yc.CASE[n].net_w, yc.CASE[n].net_h, m, b) for (n, b, m) in keys])
    return dict(zip(keys, recs))


def _where(planned, pred):
    """[(list, batch, mode, layer)] of the planned convolutions behind the first layer that satisfy pred(kernel, fields, filters, size, cin, cls)"""
    return [(n, b, m, i) for (n, b, m), rec in planned.items() for i, c in rec["convs"].items() if i > 0 and pred(*c)]


def test_every_crafted_list_is_admitted_in_every_mode(planned):
    for key, rec in planned.items():
        assert "refused" not in rec, (key, rec)
        assert sorted(rec["convs"]) == yc.CASE[key[0]].convs


def test_every_reachable_kernel_is_planned_for_a_crafted_case(planned):
    names = kernel_list()
    reached = {}
    for (n, b, m), rec in planned.items():
        for i, c in rec["convs"].items():
            reached.setdefault(c[0], []).append((n, b, m, i))
    assert set(reached) <= set(names)
    missing = [k for k in names if k not in reached and k not in UNREACHABLE]
    assert not missing, "no crafted (list, mode, batch) reaches %s" % missing
    assert not (UNREACHABLE & set(reached))


def test_the_limb_flat_kernel_never_stages_fewer_than_five_pieces():
    """k_conv3x3_b3<3, 2, 2> and <4, 2, 2> cannot be reached: the flat limb class takes the maps 81 ... 160 wide, whose staged chunk is
    (4 (128 + 2 W + 2) + 255) / 256 >= 5 pieces per thread.  Walked over every width a network can have (a network 32 W wide is W wide behind five
    stride-2 layers), with whole and partial filter tiles, at two batch sizes: the planner never yields them -- and yields <5, 2, 2> / <8, 2, 2>
    exactly on the widths 81 ... 95 / 96 ... 160."""
    widths = list(range(1, 400))
    items = []
    for W in widths:
        for F in (128, 160):
            ls = [yc.conv(32)] + [yc.conv(64, 3, 2)] * 5 + [yc.conv(F)]
            for batch in (1, 5):
                items.append((ls, 32 * W, 32, "f32x3", batch))
    recs = yc.plan_many(items)
    k = 0
    for W in widths:
        for F in (128, 160):
            for batch in (1, 5):
                kernel, f = recs[k]["convs"][6][:2]
                k += 1
                assert kernel not in UNREACHABLE, (W, F, batch)
                want = ("k_conv3x3_b3c<5>" if W <= 63 else "k_conv3x3_b3c<6>" if W <= 80 else "k_conv3x3_b3<5, 2, 2>" if W <= 95 else
                        "k_conv3x3_b3<8, 2, 2>" if W <= 160 else "k_conv_b3<2>")
                assert kernel == want and (f["width"] == W or W > 160), (W, F, batch, kernel)


def test_the_reaches_the_lists_are_built_for(planned):
    def has(what, pred):
        hits = _where(planned, pred)
        assert hits, "no crafted case plans " + what
        return hits
    has("the 32-filter f32 tile on a 3 x 3 layer", lambda k, f, F, s, cin, cls: k == "k_conv_f32<16, 1, 1, 4>" and s == 3)
    partial = {96: ("k_conv_f32<16, 2, 2, 4>", "k_conv_glds<", "k_conv_mfma<", "k_conv_b3<2>", "k_conv3x3_b3c<"),
               160: ("k_conv_f32<16, 2, 2, 4>", "k_conv_glds<", "k_conv_mfma<", "k_conv_b3<2>", "k_conv3x3_b3c<"),
               224: ("k_conv_f32<16, 2, 2, 4>", "k_conv_glds<", "k_conv_b3<2>")}
    for F, kernels in partial.items():
        for pre in kernels:
            has("a partial tile of %d filters on %s" % (F, pre), lambda k, f, FF, s, cin, cls: FF == F and k.startswith(pre))
    channels = {32: ("k_conv_f32<16", "k_conv_glds<", "k_conv_mfma<32>", "k_conv_b3<1>", "k_conv3x3_b3c<", "k_conv3x3_b3<8"),
                96: ("k_conv_f32<16", "k_conv_glds<", "k_conv_mfma<32>", "k_conv_b3<2>", "k_conv3x3_b3c<", "k_wino_gemm_f32", "k_conv3x3_flat"),
                160: ("k_conv_f32<16", "k_conv_glds<", "k_conv_b3<2>", "k_conv3x3_b3c<", "k_wino_gemm_f32", "k_conv3x3_flat")}
    for C, kernels in channels.items():
        for pre in kernels:
            has("input channels %d on %s" % (C, pre), lambda k, f, F, s, cin, cls: cin == C and k.startswith(pre))
    has("input channels 32 on k_conv3x3_glds", lambda k, f, F, s, cin, cls: cin == 32 and k.startswith("k_conv3x3_glds"))
    hits = has("k_conv3x3_b3<8, 2, 2> below width 160", lambda k, f, F, s, cin, cls: k == "k_conv3x3_b3<8, 2, 2>" and f["width"] < 160)
    assert all((4 * (128 + 2 * planned[h[:3]]["convs"][h[3]][1]["width"] + 2) + 255) // 256 in (6, 7) for h in hits)
    has("k_conv3x3_glds<160> at width 128", lambda k, f, F, s, cin, cls: k == "k_conv3x3_glds<160>")
    assert yc.CASE["wide"].net_w == 128 and ("wide", 1, "f16", 1) in _where(planned, lambda k, *_: k == "k_conv3x3_glds<160>")
    has("k_conv_mfma<32>", lambda k, *_: k == "k_conv_mfma<32>")
    routes = {(n, b, m, i): how for (n, b, m), rec in planned.items() for i, how in rec["routes"].items()}
    for m in yc.MODES:
        assert routes[("partial", 3, m, 15)] == routes[("odd", 5, m, 21)] == ("copy" if m == "f16" else "inplace"), m
        assert routes[("dense-route", 2, m, 5)] == "copy", m
    # the f16 kernels on odd maps, on maps smaller than 20 x 15 and at batches whose tiles straddle images
    f16_small = {c[0] for (n, b, m), rec in planned.items() if m == "f16" and n in ("odd", "tiny", "partial") for c in rec["convs"].values()}
    assert f16_small >= {"k_conv_first", "k_conv_glds<4, 1>", "k_conv_glds<4, 3>", "k_conv_glds<8, 1>", "k_conv_glds<8, 3>", "k_conv3x3_glds<80>", "k_conv3x3_flat",
                         "k_conv_mfma<64>", "k_conv_mfma<32>"}, f16_small
    assert len(yc.CASE["partial"].heads) == len(yc.CASE["odd"].heads) == 2 and len(yc.CASE["tiny"].heads) == 1 and not yc.CASE["no-head"].heads


def test_winograd_rule_of_the_reference_is_the_planners(planned):
    for (n, b, m), rec in planned.items():
        for i, c in rec["convs"].items():
            assert yc.CASE[n].is_wino(i, m) == (c[5] == yc.CLS_WINO), (n, b, m, i)


@pytest.mark.parametrize("mode", yc.MODES)
def test_lists_the_forward_cannot_run_are_refused_by_the_plan(mode):
    names = list(yc.REFUSED)
    recs = yc.plan_many([(yc.REFUSED[k][0], yc.REFUSED[k][1], yc.REFUSED[k][2], mode, 1) for k in names])
    for k, rec in zip(names, recs):
        assert "refused" in rec and rec["refused"][0] in (yc.SD_ERR_UNSUPPORTED, yc.SD_ERR_INVALID) and rec["refused"][1], (k, rec)


def test_weights_and_frames_are_as_the_bound_needs_them():
    for c in yc.CASES:
        payload, per = c.weights()
        cins = yc.conv_inputs(c.layers)
        assert len(payload) == sum(p["w"].size + (4 if "gamma" in p else 1) * len(p["w"]) for p in per.values())
        plain = [i for i in c.convs if not c.layers[i]["batch_normalize"]]
        assert plain, "%s: one convolution without batch norm" % c.name
        for i in c.convs:
            w = per[i]["w"]
            s = np.abs(w).max()
            assert w.shape[1] == cins[i] and np.abs(w).min() >= 0.49 * s, "every |w| within a factor two of the largest"
            if i in plain:
                assert np.array_equal(w, w.astype(np.float16).astype(np.float32)), "weights of a convolution without batch norm are f16 values"
                assert np.array_equal(c.stored(i, "f16")[0], c.stored(i, "f32")[0])
        fr = c.frames(max(c.batches))
        assert fr.dtype == np.uint8 and fr.shape[1:] == (c.net_h, c.net_w, 3)
        assert len({f.tobytes() for f in fr}) == len(fr), "every image of a batch is different"
        assert np.array_equal(c.frames(1)[0], fr[0])


def test_blob_of_a_frame_of_the_networks_size_is_the_oracles(orc):
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    for c in yc.CASES:
        fr = c.frames(1)
        want = yo.blob_from_image(fr[0], c.net_w, c.net_h, orc.resize_linear).transpose(1, 2, 0)
        assert np.array_equal(c.blobs(fr, "f32")[0], want.astype(np.float64)), c.name


def _sharp_batch(c):
    return 3 if c.name == "tiny" else max(c.batches)      # the 32 x 32 list: batch 1 has no neighbouring image, batch 96 adds nothing to three images


@pytest.fixture(scope="module")
def chains():
    """{(list, mode): {layer: LayerEval}} -- every convolution evaluated on what it reads when the layers before it are right."""
    return {}


def _chain(chains, c, mode):
    if (c.name, mode) not in chains:
        evals = {}
        c.forward_reference(c.frames(_sharp_batch(c)), mode, evals=evals)
        chains[(c.name, mode)] = evals
    return chains[(c.name, mode)]


@pytest.mark.parametrize("mode", yc.MODES)
@pytest.mark.parametrize("name", [c.name for c in yc.CASES])
def test_the_bound_rejects_every_mutant_on_every_layer(chains, name, mode):
    """Sharpness.  |mutated - ref| <= bound must FAIL for every mutation on every convolution it applies to (and every mutation applies to
    several layers of the lists: the test below)."""
    c = yc.CASE[name]
    for i, ev in _chain(chains, c, mode).items():
        bound = ev.bound()
        assert bound.shape == ev.out.shape and (bound > 0).all()
        for mut in yc.MUTATIONS:
            got = mut(ev)
            if got is None:
                continue
            bad = np.abs(got - ev.out) > bound
            assert bad.any(), "%s %s layer %d: the bound accepts %s" % (name, mode, i, mut.__name__)
    del chains[(name, mode)]          # tens of megabytes per list and mode


def test_every_mutation_applies_to_some_layer(chains):
    hit = {m.__name__: 0 for m in yc.MUTATIONS}
    for c in yc.CASES:
        for i, ev in _chain(chains, c, "f32").items():
            for m in yc.MUTATIONS:
                hit[m.__name__] += m(ev) is not None
        del chains[(c.name, "f32")]
    assert all(v >= 3 for v in hit.values()), hit


@pytest.mark.parametrize("name", [c.name for c in yc.CASES])
def test_reference_chain_agrees_with_the_oracles_float64_forward(name):
    """The float64 chain of reference_layer (mode "f64": batch norm folded in float64) is the graph oracle/yolo_oracle.torch_forward computes in
    float64 -- to float64 round-off, layer by layer and image by image; the f32-folded weights the modes store move it by a few f32 ulps."""
    import torch
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    c = yc.CASE[name]
    n = min(2, max(c.batches))
    frames = c.frames(n)
    payload, per = c.weights()
    mine = c.forward_reference(frames, "f64")
    folded = c.forward_reference(frames, "f32", storage=False)
    for k in range(n):
        blob = np.ascontiguousarray(c.blobs(frames, "f32")[k].transpose(2, 0, 1)).astype(np.float32)
        ref = yo.torch_forward(c.layers, per, blob, dtype=torch.float64)
        for i, l in enumerate(c.layers):
            if l["type"] == yc.UPSAMPLE:
                continue
            fused = l["type"] == yc.CONV and c.fused(i) is not None          # the convolution's tensor holds the shortcut's values
            want = ref[i + 1 if fused else i][0].numpy().transpose(1, 2, 0)
            got = mine[i][k]
            assert got.shape == want.shape, (name, i)
            scale = np.abs(want).max()
            assert scale > 1e-3 and np.isfinite(want).all(), (name, i, scale)
            assert np.abs(got - want).max() <= 1e-12 * scale, "%s layer %d image %d: %.3g of the layer's largest value" % (name, i, k, np.abs(got - want).max() / scale)
            assert np.abs(folded[i][k] - want).max() <= 2e-5 * scale, (name, i)


def test_crafted_heads_yield_boxes():
    """The weights are made so that the heads pass boxes through the confidence filter, NMS and the class filter -- an empty box list would
    make the GPU tests' box comparisons vacuous -- and stay below the capacities of the device path (4096 rows, 512 kept, SD_MAX_BOXES = 64)."""
    import __graft_entry__ as graft
    yo = graft.load_yolo_oracle()
    for c in yc.CASES:
        if not c.heads:
            continue
        n = min(3, max(c.batches))
        outs = c.forward_reference(c.frames(n), "f32")
        total = 0
        for k in range(n):
            rows = np.concatenate([yo.region_decode(outs[h - 1][k].astype(np.float32), list(c.layers[h]["mask"]), c.anchors, c.net_w, c.net_h) for h in c.heads])
            assert len(rows) == sum(outs[h - 1].shape[1] * outs[h - 1].shape[2] * 3 for h in c.heads)
            above = int((rows[:, 5:].max(1) > 0.5).sum())
            b, cl, cf = yo.postprocess(rows, c.net_w, c.net_h, 0.5, 0.4)
            assert above <= 2048 and len(b) <= 48, (c.name, k, above, len(b))      # the device path: 4096 rows, SD_MAX_BOXES = 64 boxes
            total += len(b)
        assert total > 0, c.name
