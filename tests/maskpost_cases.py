"""What tests/test_maskpost_cpu.py, tests/test_maskpost_gpu.py and tests/golden/make_maskpost_golden.py share: the cases of the
mask post-processing (binarise-and-resize, mask NMS), the builders of their seeded inputs, the reference's fixtures
(tests/golden/maskpost/*.npz) and the float64 band that says which pixels a test may not judge."""
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "maskpost")
MAX_EXCLUDED_SHARE = 1e-4       # of a case's pixels may lie in the band
IOU_MARGIN = 1e-4               # every mask IoU of an NMS case is at least this far from the threshold

# name: (plane set, rows, stride, crop, output size, thres).  The 25x42 planes at stride 4 give a 100x168 plane, cropped to an
# odd 97x161; the outputs are the identity, a reduction, an enlargement (rows wider than a wave's 1 KiB they are not, but 333
# bytes leave every alignment of a row start), a row narrower than one 16-byte store and a single column.
BINARIZE_CASES = {
    "identity": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (97, 161), 0.5),
    "down_60x100": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (60, 100), 0.5),
    "up_211x333": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (211, 333), 0.5),
    "narrow_97x13": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (97, 13), 0.5),
    "tiny_3x1": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (3, 1), 0.5),
    "stride2": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 2, (49, 83), (60, 100), 0.5),
    "rows_repeated_permuted": ("blobs_25x42", (5, 2, 2, 6, 0, 5, 1, 3), 4, (97, 161), (60, 100), 0.5),
    "single": ("blobs_25x42", (3,), 4, (97, 161), (97, 161), 0.5),
    "thres04": ("blobs_25x42", (0, 1, 2, 3, 4, 5, 6), 4, (97, 161), (97, 161), 0.4),
    # the two size pairs at which a float64 nearest-index rule picks other pixels than F.interpolate
    "wide_1344_to_1920": ("wide_3x336", (0, 1), 4, (11, 1344), (17, 1920), 0.5),
    "tall_800_to_1080": ("tall_200x2", (1, 0), 4, (800, 7), (1080, 5), 0.5),
}
PLANES = {"blobs_25x42": (7, 25, 42), "wide_3x336": (2, 3, 336), "tall_200x2": (2, 200, 2)}

NMS_SIZES = ((25, 42), (50, 84))            # 1050 bits (a partial last word) and 4200
NMS_COUNTS = (1, 2, 37, 300)
NMS_CASES = ["n%d_%dx%d" % (n, h, w) for h, w in NMS_SIZES for n in NMS_COUNTS]
NMS_HAND = ("two_empty", "duplicates", "chain")
NMS_THR = 0.5


def nearest_index(out, size):
    """The source index of every output index under F.interpolate(mode='nearest'): min(floor(dst * scale), in - 1) with
    scale = float32(in) / float32(out) and the product in float32."""
    scale = np.float32(size) / np.float32(out)
    idx = np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, size - 1)


def blob_planes(seed, Q, h, w):
    """Smooth blobs plus noise, [Q, h, w] float32: 1.5 x (an ellipse's signed distance in pixels) + 0.3 randn, so that a mask
    has an interior and an edge."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    planes = []
    for _ in range(Q):
        cy, cx = (0.2 + 0.6 * torch.rand(2, generator=g, dtype=torch.float64)) * torch.tensor([h, w], dtype=torch.float64)
        ry, rx = (0.15 + 0.25 * torch.rand(2, generator=g, dtype=torch.float64)) * torch.tensor([h, w], dtype=torch.float64)
        ry, rx = max(float(ry), 0.8), max(float(rx), 0.8)
        rho = torch.sqrt(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)
        planes.append(1.5 * (1.0 - rho) * min(ry, rx) + 0.3 * torch.randn(h, w, generator=g, dtype=torch.float64))
    return torch.stack(planes).float()


def _hash_noise(n, hw, seed):
    """[n, hw] float64 in [-0.5, 0.5) from an integer hash: the same numbers on every platform and library version."""
    k = np.arange(n * hw, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return ((k >> np.uint64(11)).astype(np.float64) / float(1 << 53) - 0.5).reshape(n, hw)


def nms_params(seed, n, h, w):
    """[n, 4] float64 (cy, cx, ry, rx): ellipses around a few centres, so that many of them overlap heavily, some barely.  From
    100 masks on (tens of thousands of pairs, whose IoUs would fill every 2e-4 window) they are near copies of six disjoint
    ellipses: an IoU is then either high or close to zero."""
    rng = np.random.RandomState(seed)
    if n >= 100:
        grid = np.asarray([((i + 0.5) / 2, (j + 0.5) / 3) for i in range(2) for j in range(3)])
        pick = rng.randint(0, 6, size=n)
        c = (grid[pick] + 0.006 * rng.normal(size=(n, 2))) * (h, w)
        r = (0.2, 0.155) * (1 + 0.02 * rng.normal(size=(n, 2))) * (h, w)
        return np.round(np.concatenate([c, r], 1), 3)
    centres = rng.uniform(0.2, 0.8, size=(max(2, n // 6), 2)) * (h, w)
    pick = rng.randint(0, len(centres), size=n)
    c = centres[pick] + rng.normal(0, 0.02, size=(n, 2)) * (h, w)
    r = rng.uniform(0.12, 0.3, size=(len(centres), 2))[pick] * (1 + 0.12 * rng.normal(size=(n, 2))) * (h, w)
    return np.round(np.concatenate([c, np.maximum(r, 1.0)], 1), 3)     # rounded: the stored decimals are the numbers


def nms_logits(params, h, w, seed):
    """[n, 1, h, w] float32 mask logits of the ellipses `params` with hashed noise; no logit within 0.02 of zero, so that
    sigmoid(x) > 0.5 does not depend on who computes the sigmoid."""
    params = np.asarray(params, dtype=np.float64)
    n = len(params)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cy, cx, ry, rx = (params[:, k].reshape(n, 1, 1) for k in range(4))
    rho = np.sqrt(((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2)
    x = 1.5 * (1.0 - rho) * np.minimum(ry, rx) + 0.6 * _hash_noise(n, h * w, seed).reshape(n, h, w)
    x = np.where(np.abs(x) < 0.02, np.where(x < 0, -0.02, 0.02), x)
    return torch.from_numpy(x.astype(np.float32)).view(n, 1, h, w)


def hand_logits(name, h=25, w=42):
    """Hand-built NMS cases as [n, 1, h, w] logits of +-4 and the keep flags they must give at NMS_THR."""
    def rect(x0, x1):
        m = torch.full((h, w), -4.0)
        m[5:20, x0:x1] = 4.0
        return m
    empty = torch.full((h, w), -4.0)
    if name == "two_empty":       # IoU (0 + 1e-6) / (0 + 1e-6) = 1: the later empty mask goes
        masks, keep = [empty, empty, rect(0, 20)], [True, False, True]
    elif name == "duplicates":
        masks, keep = [rect(0, 20), rect(0, 20), rect(22, 42), rect(0, 20)], [True, False, True, False]
    elif name == "chain":         # IoU(0, 1) = IoU(1, 2) = 15 / 25, IoU(0, 2) = 10 / 30: 1 goes and must not take 2 with it
        masks, keep = [rect(0, 20), rect(5, 25), rect(10, 30)], [True, False, True]
    else:
        raise KeyError(name)
    return torch.stack(masks).unsqueeze(1), keep


def mask_nms_restated(seg_masks, nms_thr):
    """mask_nms from the matrix of all pairs (numpy): (area [n], inter [n, n], keep [n] bools, the smallest distance of a
    float64 IoU from the threshold)."""
    m = (seg_masks[:, 0] > 0).reshape(len(seg_masks), -1).numpy().astype(np.float32)
    inter = np.rint(m @ m.T).astype(np.int64)
    area = np.diag(inter).copy()
    union = area[:, None] + area[None, :] - inter
    iou = ((inter.astype(np.float32) + np.float32(1e-6)) / (union.astype(np.float32) + np.float32(1e-6)))
    margin = float(np.abs((inter + 1e-6) / (union + 1e-6) - nms_thr).min())
    keep = np.ones(len(m), dtype=bool)
    for i in range(len(m)):
        if keep[i]:
            keep[i + 1:] &= ~(iou[i, i + 1:] > np.float32(nms_thr))
    return area, inter, keep, margin


@functools.lru_cache(maxsize=None)
def _npz(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def binarize_case(name):
    """dict: planes [Q, h, w] float32, rows int64 [n], stride, crop, out, thres, expect [n, H, W] uint8 (the reference's
    masks), decide [n, H, W] uint8 (the float64 decision), excluded [n, H, W] bool (the pixels in the band)."""
    plane_set, rows, stride, crop, out, thres = BINARIZE_CASES[name]
    z = _npz("binarize")
    planes = torch.from_numpy(z["planes." + plane_set])
    n = len(rows)
    expect = np.unpackbits(z[name + ".masks"], count=n * out[0] * out[1]).reshape(n, out[0], out[1])
    assert tuple(z[name + ".config"]) == (stride,) + crop + out and float(z[name + ".thres"]) == thres
    assert [int(r) for r in z[name + ".rows"]] == list(rows)
    decide, excluded = float64_decision(planes, rows, stride, crop, out, thres)
    return dict(planes=planes, rows=torch.tensor(rows, dtype=torch.int64), stride=stride, crop=crop, out=out, thres=thres,
                expect=torch.from_numpy(expect), decide=decide, excluded=excluded)


def float64_decision(planes, rows, stride, crop, out, thres):
    """The chain on doubles: the bilinear logit of every output pixel in float64, its decision against logit(thres), and the
    band 8 * 2^-23 * max(1, max |logit|) around logit(thres) inside which fp32 roundings (about three of the bilinear form and
    the sigmoid's, in logit units) may decide either way."""
    _, h, w = planes.shape
    logit = F.interpolate(planes.double()[list(rows)].unsqueeze(1), size=(h * stride, w * stride), mode="bilinear",
                          align_corners=False)[:, 0, :crop[0], :crop[1]]
    iy, ix = torch.from_numpy(nearest_index(out[0], crop[0])), torch.from_numpy(nearest_index(out[1], crop[1]))
    logit = logit[:, iy][:, :, ix]
    cut = math.log(thres / (1.0 - thres))
    band = 8.0 * 2.0 ** -23 * max(1.0, float(logit.abs().max()))
    return (logit > cut).to(torch.uint8), (logit - cut).abs() <= band


def check_masks(got, case, what):
    """`got` [n, H, W] uint8 equals the reference's masks outside the band, and the band holds at most 1e-4 of the pixels."""
    got = got.cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(case["expect"].shape), what
    share = float(case["excluded"].float().mean())
    wrong = int(((got != case["expect"]) & ~case["excluded"]).sum())
    print("%s: %d pixels, share in the band %.2e, disagreements outside it %d" % (what, got.numel(), share, wrong))
    assert share <= MAX_EXCLUDED_SHARE, (what, share)
    assert wrong == 0, (what, wrong)
    assert bool((got <= 1).all()), what


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """dict: logits [n, 1, h, w] float32, keep (the reference's list of bools), masks [n, h * w] bool (the reference's
    sigmoid > 0.5), thr."""
    z = _npz("nms")
    if name in NMS_HAND:
        logits, by_hand = hand_logits(name)
        assert [bool(k) for k in z[name + ".keep"]] == by_hand
    else:
        h, w, seed = (int(v) for v in z[name + ".geometry"])
        logits = nms_logits(z[name + ".params"], h, w, seed)
    n, _, h, w = logits.shape
    masks = np.unpackbits(z[name + ".masks"], count=n * h * w).reshape(n, h * w).astype(bool)
    return dict(logits=logits, keep=[bool(k) for k in z[name + ".keep"]], masks=torch.from_numpy(masks), thr=NMS_THR)
