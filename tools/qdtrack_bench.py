#!/usr/bin/env python
"""A/B of the QuasiDense tracker (uninext_amd/tracker.py: QuasiDenseEmbedTracker with fused = True) against the same class with
fused = False, i.e. the reference's composition, on one GPU.

    python tools/qdtrack_bench.py [--videos 5] [--frames 36]

A synthetic bdd_track-like video: about 30 or about 100 detections per frame with 256-wide embeddings, of a fixed set of objects
that come and go (each present in a frame with probability 0.85), a few near-duplicate boxes for the pre-NMS and a few
low-scoring strays that become backdrops; the tracker has the constructor arguments of the bdd_track route
(uninext_vid.py:324-336).  A video is played through a fresh tracker of each route in turn, video 0 as a warm-up; the per-frame
wall times around a device synchronisation of every frame but the first two of every other video are pooled: median and
p10 .. p90.  Nothing inside the timed region synchronises but the call itself.  "faster" means the two p10 .. p90 ranges do not
overlap.  Host synchronisations per frame are what torch.cuda.set_sync_debug_mode("warn") reports on a frame in the middle of a
video (that frame is not timed).  The ids of the two routes are compared on every frame."""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd.tracker import QuasiDenseEmbedTracker   # noqa: E402

D = 256
BDD = dict(init_score_thr=0.8, obj_score_thr=0.5, match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
           memo_momentum=1.0, nms_conf_thr=0.5, nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True,
           match_metric='bisoftmax')


def make_video(seed, objects, frames, dev):
    g = torch.Generator().manual_seed(seed)
    keys = objects + 8 * frames
    base = torch.nn.functional.normalize(torch.randn(keys, D, generator=g), dim=1)
    side = int(keys ** 0.5) + 1
    centre = torch.stack([40.0 * (torch.arange(keys) % side), 40.0 * (torch.arange(keys) // side)], 1) + 4.0 * torch.rand(keys, 2, generator=g)
    video = []
    for f in range(frames):
        present = [k for k in range(objects) if torch.rand((), generator=g) < 0.85]
        twins = present[:max(1, objects // 10)]                                   # a second, lower-scoring box on the same object
        strays = list(range(objects + 8 * f, objects + 8 * f + max(1, objects // 15)))
        which = torch.tensor(present + twins + strays)
        n = len(which)
        e = base[which] + 0.3 * torch.randn(n, D, generator=g) / D ** 0.5
        embeds = 2.8 * torch.nn.functional.normalize(e, dim=1)
        score = torch.cat([0.85 + 0.14 * torch.rand(len(present), generator=g), 0.55 + 0.2 * torch.rand(len(twins), generator=g),
                           0.2 + 0.5 * torch.rand(len(strays), generator=g)])
        c = centre[which] + 0.5 * f
        c[len(present):len(present) + len(twins)] += 1.0
        bboxes = torch.stack([c[:, 0] - 10, c[:, 1] - 8, c[:, 0] + 10, c[:, 1] + 8, score], 1)
        video.append((bboxes.to(dev), (which % 8).to(dev), embeds.to(dev), f, list(range(n))))
    return video


def play(tracker, video, times=None, probe=None):
    ids = []
    for t, fr in enumerate(video):
        torch.cuda.synchronize()
        if probe is not None and t == len(video) // 2:
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    out = tracker.match(*fr)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            probe["syncs"] = sum("synchroniz" in str(w.message).lower() for w in seen)
        else:
            t0 = time.perf_counter()
            out = tracker.match(*fr)
            torch.cuda.synchronize()
            if times is not None and t >= 2:
                times.append(1e3 * (time.perf_counter() - t0))
        ids.append((out[2].tolist(), out[3]))
    return ids


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[int(0.1 * (len(t) - 1))], t[int(0.9 * (len(t) - 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--frames", type=int, default=36)
    args = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    print("%d videos of %d frames after one warm-up video, D = %d; the bdd_track arguments of uninext_vid.py:324-336" % (args.videos, args.frames, D))
    ahead = []
    for objects in (28, 95):
        times, probes, same, dets, kept, live = ([], []), ({}, {}), True, [], [], 0
        for v in range(args.videos + 1):          # video 0 warms both routes up
            video = make_video(100 * objects + v, objects, args.frames, dev)
            dets += [len(fr[4]) for fr in video]
            got = []
            for r, fused in enumerate((True, False)):
                tracker = QuasiDenseEmbedTracker(fused=fused, **BDD)
                got.append(play(tracker, video, times[r] if v else None, probes[r] if v == 1 else None))
                if fused:
                    assert tracker._bank is not None, "the kernels did not take the call"
                    live = max(live, tracker._bank.count)
            kept += [len(ids) for ids, _ in got[0]]
            same = same and got[0] == got[1]
        (mf, lf, hf), (mc, lc, hc) = stats(times[0]), stats(times[1])
        verdict = "fused faster" if hf < lc else ("composition faster" if hc < lf else "ranges overlap")
        ahead.append(verdict == "fused faster" and same)
        print("  %.0f detections per frame, %.0f after the pre-NMS (up to %d live tracklets), %d timed frames per route:"
              % (sum(dets) / len(dets), sum(kept) / len(kept), live, len(times[0])))
        print("      fused       %8.3f ms per frame (p10 %.3f .. p90 %.3f), %s host syncs" % (mf, lf, hf, probes[0].get("syncs")))
        print("      composition %8.3f ms per frame (p10 %.3f .. p90 %.3f), %s host syncs   x%.1f  %s; ids and indices %s"
              % (mc, lc, hc, probes[1].get("syncs"), mc / mf, verdict, "equal on every frame" if same else "DIFFER"), flush=True)
    print("fused faster at both sizes with equal ids: %s" % ("yes" if all(ahead) else "no"))


if __name__ == "__main__":
    main()
