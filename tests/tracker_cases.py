"""What tests/test_tracker_cpu.py, tests/test_tracker_gpu.py and tests/golden/make_tracker_golden.py share: the seeded
sequences the online tracker is tested on, and the reference's recorded answers (tests/golden/tracker/<case>.npz).

A sequence is a script: per frame a list of detections (key, score, cell, shift).  `key` picks one vector of an orthonormal
basis (an object, or clutter that never scores high); the detection's embedding is that vector plus seeded noise, scaled to
norm 0.98 sqrt(8), so that |embeds . memo^T| <= 8 whatever the memory has averaged (the reference's embeddings give logits of
this order).  ('mix', a, b, wa, wb) blends two keys.  The mask logits are 12x20 (240 pixels, not a multiple of 32), +4 on the 1x3
rectangle of `cell` moved `shift` pixels to the right and -4 elsewhere: shift 0 twice is a duplicate (IoU 1), shift 1 overlaps
the cell's own rectangle with IoU 2/4, shift 2 with 1/5.

Every case must keep a float64 margin of MARGIN on every decision of every frame (tests/tracker_ref.py measures it,
tests/test_tracker_cpu.py asserts it): a condition on the inputs, met by choosing the seed, not a tolerance on the kernels."""
import functools
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tracker")
MARGIN = 1e-3
H, W = 12, 20
CELLS_PER_ROW = 6
EMBED_NORM = 0.98 * 8.0 ** 0.5
NOISE = 0.3


def _objects(keys, score=0.9):
    return [(k, score, k, 0) for k in keys]


def _waves():
    """n = 63, 64, 65, 1 detections; the memory grows 63 -> 64 -> 65 slots, so rows and columns cross a wave of 64."""
    return [_objects(range(63)), _objects(range(64)), _objects(range(65)), _objects(range(65)), _objects([7]),
            _objects(reversed(range(65))), _objects(range(63)), _objects(range(65))]


def _bookkeeping():
    """memo_tracklet_frames = 3, memory_len = 3.  Object 0 is seen six times running (the ring wraps), 1 vanishes for one frame, 2
    for two (back with a velocity divisor of 3), 3 for three (expired: a new identity); three frames of clutter empty the memory,
    and the frame after takes the empty-memory branch, where 0.3 is above init_score_thr though below addnew_score_thr."""
    clutter = lambda f: [(10 + 3 * f + j, 0.1, 20 + 2 * j, 0) for j in range(3)]
    return [_objects([0, 1, 2, 3]), _objects([0, 1]), _objects([0]), _objects([0, 1, 2]), _objects([0, 1, 2, 3]), _objects([0, 1, 2]),
            clutter(0), clutter(1), clutter(2), [(0, 0.9, 0, 0), (1, 0.3, 1, 0)], _objects([0, 1])]


def _decisions():
    """Frame 2: the first detection is unselected with nothing before it (a backdrop); one below addnew_score_thr overlaps object
    0's mask (stays -2), one does not (a backdrop), its duplicate goes in the pre-NMS.  Frame 6: two detections of object 0
    compete for its tracklet; the loser finds the column zeroed and starts a tracklet of its own."""
    return [_objects([0, 2, 4]), _objects([0, 2, 4]),
            [(20, 0.3, 30, 0), (0, 0.9, 0, 0), (21, 0.3, 0, 1), (22, 0.3, 40, 0), (23, 0.9, 40, 0), (2, 0.9, 2, 0), (4, 0.9, 4, 0)],
            _objects([0, 2, 4, 6]), _objects([2, 0, 6, 4]), _objects([0, 2, 4, 6]),
            [(0, 0.9, 0, 0), (0, 0.9, 50, 0), (2, 0.9, 2, 0)], _objects([2, 4])]


def _frame_weight():
    """frame_weight.  Object 0 has been seen five times and object 2 twice when frame 5 brings a detection between the two,
    nearer to 2: both scores are above 0.5, the plain maximum is 2's column, the maximum weighted by exist_frame is 0's."""
    return [_objects([0, 4]), _objects([0, 4]), _objects([0, 4]), _objects([0, 2, 4]), _objects([0, 2, 4]),
            [(("mix", 0, 2, 0.69, 0.72), 0.9, 0, 0), (4, 0.9, 4, 0)], _objects([0, 2, 4]), _objects([0, 2, 4])]


def _grow():
    """Two, two, then three and more detections: with capacity = 4 the third frame no longer fits the device bank."""
    return [_objects([0, 1]), _objects([0, 1]), _objects([0, 1, 2]), _objects([0, 1, 2, 3, 4]), _objects([4, 3, 2, 1, 0]),
            _objects([0, 2, 4, 5]), _objects([0, 1, 2, 3, 4, 5]), _objects([5, 0])]


def _d8():
    return [_objects([0, 1, 2]), _objects([0, 1, 2, 3]), [(5, 0.3, 30, 0), (0, 0.9, 0, 0), (1, 0.9, 1, 0), (6, 0.3, 40, 0)],
            _objects([3, 2, 1, 0]), _objects([0, 4]), _objects([0, 1, 2, 3, 4]), _objects([4]), _objects([0, 1, 2, 3, 4])]


# name: (script, embedding width, seed, constructor arguments)
CASES = {
    "waves": (_waves, 256, 1, {}),
    "bookkeeping": (_bookkeeping, 256, 1, dict(memo_tracklet_frames=3, memory_len=3)),
    "bookkeeping_long": (_bookkeeping, 256, 1, dict(memo_tracklet_frames=3, memory_len=3, long_match=True)),
    "bookkeeping_long_temporal": (_bookkeeping, 256, 1, dict(memo_tracklet_frames=3, memory_len=3, long_match=True,
                                                              temporal_weight=True)),
    "decisions": (_decisions, 256, 1, {}),
    "frame_weight": (_frame_weight, 256, 1, dict(frame_weight=True)),
    "grow": (_grow, 256, 1, {}),
    "d8": (_d8, 8, 1, {}),
}
OVERFLOW_CASE, OVERFLOW_CAPACITY = "grow", 4


def _basis(seed, D, count):
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(D, D, generator=g, dtype=torch.float64))
    if count <= D:
        return q.t()[:count]
    extra = torch.randn(count - D, D, generator=g, dtype=torch.float64)
    return torch.cat([q.t(), extra / extra.norm(dim=1, keepdim=True)])


def _key_count(script):
    top = 0
    for frame in script:
        for key, _, _, _ in frame:
            top = max(top, max(key[1], key[2]) if isinstance(key, tuple) else key)
    return top + 1


def mask_logits(cell, shift):
    m = torch.full((H, W), -4.0)
    r, x0 = (cell // CELLS_PER_ROW) % H, 3 * (cell % CELLS_PER_ROW) + shift
    m[r, x0:x0 + 3] = 4.0
    return m


@functools.lru_cache(maxsize=None)
def frames(name, seed=None):
    """The case's frames: a list of dict(bboxes [n, 5], labels [n] int64, masks [n, 1, 12, 20], embeds [n, D], frame_id, indices)
    of fp32 CPU tensors.  Shared: callers must not write into them."""
    script, D, case_seed, _ = CASES[name]
    script = script()
    seed = case_seed if seed is None else seed
    basis = _basis(seed, D, _key_count(script))
    g = torch.Generator().manual_seed(seed + 7919)
    out = []
    for f, frame in enumerate(script):
        bboxes, labels, masks, embeds = [], [], [], []
        for key, score, cell, shift in frame:
            if isinstance(key, tuple):
                base, label = key[3] * basis[key[1]] + key[4] * basis[key[2]], key[1] % 5
            else:
                base, label = basis[key], key % 5
            noise = torch.randn(D, generator=g, dtype=torch.float64) / D ** 0.5
            e = base / base.norm() + NOISE * noise
            embeds.append(EMBED_NORM * e / e.norm())
            x, y = 10.0 * (cell % CELLS_PER_ROW) + 0.5 * f + shift, 8.0 * (cell // CELLS_PER_ROW) + 0.25 * f
            bboxes.append([x, y, x + 9.0, y + 6.0, score])
            labels.append(label)
            masks.append(mask_logits(cell, shift))
        n = len(frame)
        out.append(dict(bboxes=torch.tensor(bboxes, dtype=torch.float64).float().view(n, 5), labels=torch.tensor(labels, dtype=torch.int64),
                        masks=torch.stack(masks).view(n, 1, H, W), embeds=torch.stack(embeds).float().view(n, D), frame_id=f,
                        indices=[7 * i + 3 for i in range(n)]))
    return out


def run(tracker, name, device="cpu", upto=None, frames_=None):
    """Drive `tracker` through the case; returns per frame (ids list, indices, kept count)."""
    out = []
    for fr in (frames_ or frames(name))[:upto]:
        b, l, ids, ind = tracker.match(fr["bboxes"].to(device), fr["labels"].to(device), fr["masks"].to(device), fr["embeds"].to(device),
                                       fr["frame_id"], list(fr["indices"]))
        assert b.shape[0] == l.shape[0] == ids.shape[0] == len(ind) and ids.dtype == torch.int64 and not ids.is_cuda
        assert isinstance(ind, list)
        out.append((ids.tolist(), ind, len(ind)))
    return out


MEMO_NAMES = ("bboxes", "labels", "embeds", "ids", "vs", "long_embeds", "long_score", "exist_frame")


def memo_arrays(memo):
    """The 8-tuple of `memo` as {name: float64 / int64 numpy array}; the two lists of rings are concatenated, and the rings'
    lengths are added as `long_len`."""
    out = {}
    for name, t in zip(MEMO_NAMES, memo):
        if isinstance(t, (list, tuple)):
            if name == "long_embeds":
                out["long_len"] = np.asarray([len(x) for x in t], dtype=np.int64)
            t = torch.cat([x.reshape(len(x), -1) for x in t], 0) if len(t) else torch.zeros(0, 1)
        t = t.detach().cpu()
        out[name] = t.numpy().astype(np.float64 if t.is_floating_point() else np.int64)
    return out


def assert_memo_close(got, want, what, tol=1e-4):
    """Every tensor of `got` within tol x the magnitude of that tensor in `want`; integers equal."""
    assert set(got) == set(want), what
    for name in want:
        a, b = got[name], want[name]
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        if b.dtype == np.int64:
            assert np.array_equal(a, b), (what, name)
        elif b.size:
            err, scale = float(np.abs(a - b).max()), max(float(np.abs(b).max()), 1e-30)
            print("%s %-12s max error %.3e of magnitude %.3e" % (what, name, err, scale))
            assert err <= tol * scale, (what, name, err, scale)


@functools.lru_cache(maxsize=None)
def golden(name):
    """The reference's record of the case: dict(frames=[(ids, indices, kept)], memo={...}, seed)."""
    with np.load(os.path.join(GOLDEN, "%s.npz" % name)) as z:
        count = int(z["frames"])
        fr = [([int(v) for v in z["%d.ids" % t]], [int(v) for v in z["%d.indices" % t]], int(z["kept"][t])) for t in range(count)]
        memo = {k[5:]: z[k] for k in z.files if k.startswith("memo.")}
        return dict(frames=fr, memo=memo, seed=int(z["seed"]))
