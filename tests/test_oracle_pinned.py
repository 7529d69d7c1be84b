"""Pins the CPU oracle (oracle/yolo_oracle.py) against outputs of the REFERENCE itself, recorded in
tests/golden/*.npz by tests/golden/make_golden.py.  Runs on the CPU; no GPU, no reference needed."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import yolo_oracle as orc

torch.set_num_threads(8)


def T(a):
    return torch.from_numpy(np.array(a))


def exact_sum(t):
    """Correctly rounded float64 sum (math.fsum): the same bits on every CPU, whatever order a vectorised sum would take."""
    return math.fsum(t.detach().double().reshape(-1).tolist())


def close(a, b, rtol=1e-5, atol=1e-6):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol)


# ---- F1: building blocks ---------------------------------------------------------------------------
def _block_params(g, name):
    pre = f"{name}/init/"
    return {k[len(pre):]: T(g[k]).clone() for k in g.files if k.startswith(pre)}


def _run_block(name, P, x, training):
    n = orc._Net(P, training)
    if name.startswith("cb"):
        stride = 2 if name.endswith("s2") else 1
        Pp = {f"b.{k}": v for k, v in P.items()}
        return orc._Net(Pp, training).cbs(x, "b", stride), Pp
    Pp = {f"b.{k}": v for k, v in P.items()}
    n = orc._Net(Pp, training)
    if name == "bneck":
        return n.bottleneck(x, "b"), Pp
    if name.startswith("c3"):
        return n.c3(x, "b"), Pp
    return n.sppf(x, "b"), Pp


@pytest.mark.parametrize("name", ["cb3x3", "cb3x3s2", "cb1x1", "bneck", "c3", "c3wide", "sppf"])
def test_blocks_match_reference(name):
    g = load_golden("blocks")
    P = _block_params(g, name)
    for k, v in P.items():
        if v.dtype.is_floating_point and "running" not in k:
            v.requires_grad_(True)
    x = T(g[f"{name}/x"]).clone().requires_grad_(True)
    y, Pp = _run_block(name, P, x, True)
    close(y.detach(), g[f"{name}/y"], 1e-4, 1e-5)
    (y * T(g[f"{name}/w"])).sum().backward()
    close(x.grad, g[f"{name}/dx"], 1e-3, 1e-5)
    for k in g.files:
        if k.startswith(f"{name}/grad/"):
            close(Pp["b." + k.split("/grad/")[1]].grad, g[k], 2e-3, 2e-5)
        if k.startswith(f"{name}/after/"):
            close(Pp["b." + k.split("/after/")[1]].detach(), g[k], 1e-5, 1e-6)
    with torch.no_grad():
        y_eval, _ = _run_block(name, {k: v.detach() for k, v in P.items()}, x.detach(), False)
    close(y_eval, g[f"{name}/y_eval"], 1e-4, 1e-5)


# ---- F2 / F3 / F4: decode, CIoU, losses ----------------------------------------------------------------
def test_decode_matches_reference():
    g = load_golden("decode")
    for key in ("nc1_img640", "nc1_img1280", "nc3_img640", "nc3_img1280"):
        img = int(key.split("img")[1])
        close(orc.decode(T(g[f"{key}/raw"]), T(g[f"{key}/anchors"]), img), g[f"{key}/decoded"], 1e-6, 1e-7)
    close(orc.decode(T(g["default/raw"]), T(g["default/anchors"])), g["default/decoded"], 1e-6, 1e-7)


@pytest.mark.parametrize("case", ["identical", "disjoint", "partial", "aspect", "contained", "rand"])
def test_ciou_matches_reference(case):
    g = load_golden("ciou")
    p = T(g[f"{case}/pred"]).clone().requires_grad_(True)
    l = orc.ciou(p, T(g[f"{case}/tgt"]))
    l.backward()
    close(l.detach(), g[f"{case}/loss"], 1e-6, 1e-7)
    close(p.grad, g[f"{case}/dpred"], 1e-5, 1e-7)


def loss_inputs(tag):
    """Rebuilds the seeded inputs of make_golden.gen_loss (inputs are generated, outputs are golden)."""
    g = load_golden("loss")
    nc = 3 if tag == "nc3" else 1
    seed = int(g[f"{tag}/seed"][0])
    torch.manual_seed(seed)
    preds = [(torch.randn(2, gs, gs, 3, 5 + nc) * 1.5) for gs in (80, 40, 20)]
    targets = [torch.zeros(2, gs, gs, 3, 5 + nc) for gs in (80, 40, 20)]
    for s in range(3):
        idx, val = g[f"{tag}/s{s}/pos_idx"], g[f"{tag}/s{s}/pos_tgt"]
        for (b, i, j, a), v in zip(idx, val):
            targets[s][b, i, j, a] = T(v)
    return g, nc, preds, targets


@pytest.mark.parametrize("tag", ["nc1", "nc3", "nc1_empty"])
def test_multiscale_loss_matches_reference(tag):
    g, nc, preds, targets = loss_inputs(tag)
    preds = [p.requires_grad_(True) for p in preds]
    anchors = [torch.tensor(a, dtype=torch.float32) for a in orc.DEFAULT_ANCHORS]
    tot, b, o, c = orc.loss_multiscale(preds, targets, anchors, nc)
    close([float(tot), float(b), float(o), float(c)], g[f"{tag}/scalars"], 1e-6, 1e-7)
    tot.backward()
    for s, p in enumerate(preds):
        per = [float(v) for v in orc.loss_one_scale(p.detach(), targets[s], anchors[s], nc)]
        close(per, g[f"{tag}/per_scale"][s], 1e-6, 1e-7)
        close(p.grad.reshape(-1)[T(g[f"{tag}/s{s}/sample_idx"])], g[f"{tag}/s{s}/dpred_sample"], 1e-5, 1e-9)
        if f"{tag}/s{s}/dpred_pos" in g.files:
            close(p.grad[targets[s][..., 4] > 0.5], g[f"{tag}/s{s}/dpred_pos"], 1e-5, 1e-9)


# ---- target assignment ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3])
def test_assignment_rule_matches_reference_dataset(nc):
    g = load_golden("assign")
    labels = g[f"nc{nc}/labels"]
    boxes = [[(int(r[0]), *map(float, r[1:])) for r in img] for img in labels]
    tg = orc.assign_targets(boxes, 640, nc)
    for b in range(3):
        for s in range(3):
            pos = tg[s][b][..., 4] > 0.5
            np.testing.assert_array_equal(pos.nonzero().numpy(), g[f"nc{nc}/b{b}/s{s}/idx"])
            close(tg[s][b][pos], g[f"nc{nc}/b{b}/s{s}/val"], 1e-6, 1e-7)


# ---- NMS ------------------------------------------------------------------------------------------------
def test_python_nms_restatement_matches_reference():
    g = load_golden("nms")
    for M in (1, 3, 64, 300, 1000):
        boxes, scores = g[f"M{M}/boxes"], g[f"M{M}/scores"]
        dets = [(float(b[0]), float(b[1]), float(b[2]), float(b[3]), float(s), 0) for b, s in zip(boxes, scores)]
        for thr in (0.4, 0.6):
            kept = orc.nms_python(dets, thr)
            idx = [dets.index(d) for d in kept]
            np.testing.assert_array_equal(idx, g[f"M{M}_t{thr}/kept"])
    ka = [tuple(r) for r in g["ka3/dets"]]
    assert [ka.index(d) for d in orc.nms_python(ka, 0.5)] == list(g["ka3/kept"]) == [0, 2]
    ka2 = [tuple(r) for r in g["ka2/dets"]]
    assert [ka2.index(d) for d in orc.nms_python(ka2, 0.3)] == list(g["ka2/kept_0.3"])
    assert [ka2.index(d) for d in orc.nms_python(ka2, 0.7)] == list(g["ka2/kept_0.7"])
    assert abs(orc.iou_corners((0, 0, 10, 10), (5, 0, 15, 10)) - float(g["iou/half_shift"][0])) < 1e-12


def test_batched_nms_definition_agrees_with_reference_python_nms_single_class():
    """Class-aware NMS is unpinned by the reference (torchvision absent); for ONE class and no pair
    on the threshold it must select exactly what the reference's python nms() selects."""
    g = load_golden("nms")
    for M in (3, 64, 300, 1000):
        boxes, scores = g[f"M{M}/boxes"], g[f"M{M}/scores"]
        for thr in (0.4, 0.6):
            kept = orc.nms_batched(boxes, scores, np.zeros(M, np.int64), thr)
            np.testing.assert_array_equal(kept, g[f"M{M}_t{thr}/kept"])


def test_batched_nms_is_class_aware_and_stable():
    b = np.array([[0, 0, 10, 10], [1, 1, 11, 11], [0, 0, 10, 10], [50, 50, 60, 60]], np.float32)
    s = np.array([0.9, 0.8, 0.9, 0.1], np.float32)
    assert list(orc.nms_batched(b, s, np.array([0, 0, 0, 0]), 0.5)) == [0, 3]        # tie -> lower index first
    assert list(orc.nms_batched(b, s, np.array([0, 1, 2, 0]), 0.5)) == [0, 2, 1, 3]  # other classes survive
    assert list(orc.nms_batched(np.zeros((0, 4)), np.zeros(0), np.zeros(0), 0.5)) == []


def _nms_bruteforce(boxes, scores, thr):
    """Independent scalar re-statement of torchvision's CPU nms loop (python floats rounded through np.float32)."""
    f = np.float32
    order = sorted(range(len(scores)), key=lambda k: (-float(scores[k]), k))
    dead, kept = set(), []
    for a, i in enumerate(order):
        if i in dead:
            continue
        kept.append(i)
        ai = f(f(boxes[i, 2] - boxes[i, 0]) * f(boxes[i, 3] - boxes[i, 1]))
        for j in order[a + 1:]:
            if j in dead:
                continue
            w = max(f(0), f(min(boxes[i, 2], boxes[j, 2]) - max(boxes[i, 0], boxes[j, 0])))
            h = max(f(0), f(min(boxes[i, 3], boxes[j, 3]) - max(boxes[i, 1], boxes[j, 1])))
            inter = f(w * h)
            aj = f(f(boxes[j, 2] - boxes[j, 0]) * f(boxes[j, 3] - boxes[j, 1]))
            with np.errstate(divide="ignore", invalid="ignore"):
                ovr = f(inter / f(f(ai + aj) - inter))
            if float(ovr) > thr:
                dead.add(j)
    return kept


def test_batched_nms_both_torchvision_branches():
    """The two branches of torchvision.ops.batched_nms and the size rule that picks one (oracle header).  Unpinned by the
    reference; held here to an independent scalar restatement and to constructed cases whose answer is known by hand."""
    rng = np.random.default_rng(7)
    for M, nc in ((40, 3), (200, 80), (300, 5)):
        ctr, wh = rng.uniform(-20, 300, (M, 2)), rng.uniform(8, 120, (M, 2))
        b = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(np.float32)
        sc = rng.uniform(0.01, 1, M).astype(np.float32)
        sc[rng.integers(0, M, M // 4)] = sc[rng.integers(0, M, M // 4)]
        cl = rng.integers(0, nc, M)
        shifted = orc.nms_shifted_boxes(b, cl)
        unit = np.float32(b.max() + np.float32(1))
        np.testing.assert_array_equal(shifted, (b + (cl.astype(np.float32) * unit).astype(np.float32)[:, None]).astype(np.float32))
        assert list(orc.nms_batched(b, sc, cl, 0.4, "trick")) == _nms_bruteforce(shifted, sc, 0.4)
        per_class = []
        for c in np.unique(cl):
            idx = np.nonzero(cl == c)[0]
            per_class += [int(idx[k]) for k in _nms_bruteforce(b[idx], sc[idx], 0.4)]
        per_class.sort(key=lambda k: (-float(sc[k]), k))
        assert list(orc.nms_batched(b, sc, cl, 0.4, "vanilla")) == per_class
        assert list(orc.nms_batched(b, sc, cl, 0.4)) == list(orc.nms_batched(b, sc, cl, 0.4, "trick"))   # M <= 1000: trick
        z = np.zeros(M, np.int64)                                                 # one class: offsets are 0, branches agree
        assert list(orc.nms_batched(b, sc, z, 0.4, "trick")) == list(orc.nms_batched(b, sc, z, 0.4, "vanilla"))
    # size rule: numel = 4 M, > 4000 (CPU tensors) / > 20000 (GPU tensors) -> per class
    assert orc.nms_uses_trick(1000, "cpu") and not orc.nms_uses_trick(1001, "cpu")
    assert orc.nms_uses_trick(5000, "cuda") and not orc.nms_uses_trick(5001, "cuda")
    # the threshold is a C double: an IoU of exactly float32(0.4) = 0.4000000059... is above 0.4
    b = np.array([[0, 0, 3.5, 1], [1.5, 0, 5, 1]], np.float32)                    # inter 2, union 5
    s2 = np.array([0.9, 0.8], np.float32)
    for mode in ("vanilla", "trick"):
        assert list(orc.nms_batched(b, s2, [0, 0], 0.4, mode)) == [0]
        assert list(orc.nms_batched(b, s2, [0, 0], float(np.float32(0.4)), mode)) == [0, 1]
    # the branches DIFFER for nc > 1: (i) negative coordinates reach into the previous class's band ...
    b = np.array([[600, 600, 640, 640], [-41, -41, -1, -1]], np.float32)          # class 1 shifted by 641 lands on class 0's box
    assert list(orc.nms_batched(b, s2, [0, 1], 0.4, "vanilla")) == [0, 1]
    assert list(orc.nms_batched(b, s2, [0, 1], 0.4, "trick")) == [0]
    # ... (ii) the shifted coordinates round on a coarser grid (ulp 0.004 at 79 * 641): a pair just below the threshold
    # unshifted is above it after the shift (found by search, values are exact float32)
    b = np.array([[303.3179016113281, 364.748291015625, 337.342529296875, 374.748291015625],
                  [317.89996337890625, 364.748291015625, 351.92462158203125, 374.748291015625], [0, 0, 640, 1]], np.float32)
    s3, c3 = np.array([0.9, 0.8, 0.1], np.float32), np.array([79, 79, 0])
    assert list(orc.nms_batched(b, s3, c3, 0.4, "vanilla")) == [0, 1, 2]
    assert list(orc.nms_batched(b, s3, c3, 0.4, "trick")) == [0, 2]


# ---- F8: candidate extraction --------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["nc1_sq", "nc3_rect"])
def test_candidates_match_reference_predict(tag):
    g = load_golden("candidates")
    nc, img, thr, scale, pad_top, pad_left = g[f"{tag}/meta"]
    preds = [T(g[f"{tag}/pred{s}"]) for s in range(3)]
    anchors = [T(a) for a in g[f"{tag}/anchors"]]
    boxes, scores, classes = orc.candidates(preds, anchors, int(img), int(nc), float(thr), pad_left, pad_top, scale)
    np.testing.assert_array_equal(classes.numpy(), g[f"{tag}/classes"])
    close(scores, g[f"{tag}/scores"], 1e-6, 1e-8)
    close(boxes, g[f"{tag}/boxes"], 1e-6, 1e-4)


# ---- F5 / F6: the full model -----------------------------------------------------------------------------
def _product_state(nc, S):
    """Seeded parameters: the product's module tree reproduces the reference's initial weights bit for
    bit (checked here through the golden per-tensor checksums)."""
    import yolo_from_scratch_amd as y
    torch.manual_seed(0)
    m = y.YOLO(num_classes=nc, img_size=S)
    return m


@pytest.mark.parametrize("tag,nc,S", [("model_nc1", 1, 640), ("model_nc3", 3, 320)])
def test_full_model_step_matches_reference(tag, nc, S):
    g = load_golden(tag)
    m = _product_state(nc, S)
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    close([exact_sum(v) for v in sd.values()], g["init_sum"], 0, 0)
    close([exact_sum(v.abs()) for v in sd.values()], g["init_abs"], 0, 0)
    P = {k: v.clone() for k, v in sd.items()}
    names = list(g["param_names"])
    for n in names:
        P[n].requires_grad_(True)
    x = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(123))
    close(exact_sum(x), g["x_sum"][0], 0, 0)
    targets = orc.assign_targets(orc.synthetic_boxes(2, nc, S, 8, 2000), S, nc)
    preds = orc.forward(P, x, nc, training=True)
    tot, b, o, c = orc.loss_multiscale(preds, targets, orc.anchors_of(P), nc)
    close([float(tot), float(b), float(o), float(c)], g["scalars"], 2e-5, 1e-6)
    for s, p in enumerate(preds):
        close(p.detach().reshape(-1)[T(g[f"pred{s}_idx"])], g[f"pred{s}_sample"], 1e-3, 1e-4)
        # decoded boxes of the whole forward at the reference's sampled cells: north_star's "fp32 boxes within 1e-4 relative"
        dec = orc.decode(p.detach(), orc.anchors_of(P)[s], S).reshape(-1, 5 + nc)[T(g[f"dec{s}_cells"]), :4]
        close(dec, g[f"dec{s}_boxes"], 1e-4, 1e-6)
    tot.backward()
    gn = np.array([float(P[n].grad.double().norm()) for n in names])
    q2 = {"stem.0.bias", "stem.3.bias", "backbone_p3.1.bias", "backbone_p4.0.bias", "backbone_p5.0.bias",
          "sppf.conv1.bias", "sppf.conv2.bias"}          # biases in front of BN: pure rounding noise (quirk Q2)
    live = np.array([n not in q2 for n in names])
    close(gn[live], g["grad_norm"][live], 2e-3, 1e-6)
    total, coef = orc.clip_coef([P[n].grad for n in names])
    close(total, g["total_grad_norm"][0], 1e-4, 0)
    for k in g.files:
        if k.startswith("bn/"):
            close(P[k[3:]], g[k], 1e-4, 1e-6)
    # clip + Adam, then the second forward's loss
    with torch.no_grad():
        for n in names:
            gr = P[n].grad * coef
            orc.adam_step(P[n], gr, torch.zeros_like(gr), torch.zeros_like(gr), 1, 1e-3)
    preds = orc.forward({k: v.detach() for k, v in P.items()}, x, nc, training=True)
    tot2 = orc.loss_multiscale(preds, targets, orc.anchors_of(P), nc)
    close([float(v) for v in tot2], g["scalars_step2"], 5e-4, 1e-5)
