#!/usr/bin/env python
"""A/B of the online tracker (uninext_amd/tracker.py: IDOL_Tracker with fused = True) against the same class with fused = False,
i.e. the reference's composition (with this package's mask_nms for the pre-NMS on both routes), on one GPU.

    python tools/tracker_bench.py [--videos 5] [--frames 36]

A synthetic video: about 30 or about 100 detections per frame of 200x336 mask logits and 256-wide embeddings, of a fixed set of
objects that come and go (each present in a frame with probability 0.85) plus a few low-scoring strays; the tracker has the VIS
settings of uninext_vid.py:338-350, once with the long-match flags off and once with long_match, frame_weight and temporal_weight
on (memory_len 3).  A video is played through a fresh tracker of each route in turn; the per-frame wall times around a device
synchronisation of every frame but the first two of every video are pooled: median and p10..p90 spread; "faster" means the
medians differ by more than the larger spread.  Host synchronisations per frame are what torch.cuda.set_sync_debug_mode("warn")
reports on a frame in the middle of a video; temporaries are the allocator's high-water mark of such a frame above what was
allocated before it."""
import argparse
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uninext_amd.tracker import IDOL_Tracker   # noqa: E402

H, W, D = 200, 336, 256
VIS = dict(init_score_thr=0.2, obj_score_thr=0.1, nms_thr_pre=0.5, nms_thr_post=0.05, addnew_score_thr=0.2, memo_tracklet_frames=10,
           memo_momentum=0.8)
LONG = dict(long_match=True, frame_weight=True, temporal_weight=True, memory_len=3)


def make_video(seed, objects, frames, dev):
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.normalize(torch.randn(objects + 8 * frames, D, generator=g), dim=1)
    centre = torch.rand(objects + 8 * frames, 2, generator=g) * torch.tensor([H - 40.0, W - 40.0]) + 20.0
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    video = []
    for f in range(frames):
        present = [k for k in range(objects) if torch.rand((), generator=g) < 0.85]
        strays = list(range(objects + 8 * f, objects + 8 * f + max(1, objects // 15)))
        keys = torch.tensor(present + strays)
        n = len(keys)
        e = base[keys] + 0.3 * torch.randn(n, D, generator=g) / D ** 0.5
        embeds = 2.8 * torch.nn.functional.normalize(e, dim=1)
        score = torch.cat([0.5 + 0.5 * torch.rand(len(present), generator=g), 0.05 + 0.1 * torch.rand(len(strays), generator=g)])
        c = centre[keys] + 0.5 * f
        r = 6.0 + 4.0 * torch.rand(n, 1, 1, generator=g)
        rho = torch.sqrt((ys - c[:, 0, None, None]) ** 2 + (xs - c[:, 1, None, None]) ** 2)
        masks = (1.5 * (r - rho)).unsqueeze(1)
        bboxes = torch.stack([c[:, 1] - 8, c[:, 0] - 8, c[:, 1] + 8, c[:, 0] + 8, score], 1)
        video.append((bboxes.to(dev), (keys % 40).to(dev), masks.to(dev), embeds.to(dev), f, list(range(n))))
    return video


def play(tracker, video, times=None, probe=None):
    ids = []
    for t, fr in enumerate(video):
        torch.cuda.synchronize()
        if probe is not None and t == len(video) // 2:
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    out = tracker.match(*fr)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            probe["syncs"] = sum("synchroniz" in str(w.message).lower() for w in seen)
            probe["peak"] = torch.cuda.max_memory_allocated() - base
        else:
            t0 = time.perf_counter()
            out = tracker.match(*fr)
            torch.cuda.synchronize()
            if times is not None and t >= 2:
                times.append(1e3 * (time.perf_counter() - t0))
        ids.append(out[2].tolist())
    return ids


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[int(0.9 * (len(t) - 1))] - t[int(0.1 * (len(t) - 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=5)
    ap.add_argument("--frames", type=int, default=36)
    args = ap.parse_args()
    dev = "cuda:0"
    print(torch.cuda.get_device_name(0), "torch", torch.__version__)
    print("%d-frame videos, %dx%d mask logits, D = %d; VIS settings of uninext_vid.py:338-350" % (args.frames, H, W, D))
    ahead = []
    for label, extra in (("long-match flags off", {}), ("long_match + frame_weight + temporal_weight, memory_len 3", LONG)):
        for objects in (32, 105):
            times, probes, same, dets, live = ([], []), ({}, {}), True, [], 0
            for v in range(args.videos + 1):          # video 0 warms both routes up
                video = make_video(100 * objects + v, objects, args.frames, dev)
                dets += [len(fr[5]) for fr in video]
                got = []
                for r, fused in enumerate((True, False)):
                    tracker = IDOL_Tracker(fused=fused, **VIS, **extra)
                    got.append(play(tracker, video, times[r] if v else None, probes[r] if v == 1 else None))
                    if fused:
                        assert tracker._bank is not None, "the kernels did not take the call"
                        live = max(live, tracker._bank.count)
                same = same and got[0] == got[1]
            (tf, sf), (tt, st) = stats(times[0]), stats(times[1])
            verdict = "fused faster" if tt - tf > max(sf, st) else ("composition faster" if tf - tt > max(sf, st) else "within spread")
            ahead.append(verdict == "fused faster")
            print("  %s, %.0f detections per frame (up to %d live tracklets):" % (label, sum(dets) / len(dets), live))
            print("      fused       %8.3f ms per frame (spread %.3f), %s host syncs, %.2f MB of temporaries" %
                  (tf, sf, probes[0].get("syncs"), probes[0].get("peak", 0) / 1e6))
            print("      composition %8.3f ms per frame (spread %.3f), %s host syncs, %.2f MB of temporaries   x%.1f  %s; ids %s" %
                  (tt, st, probes[1].get("syncs"), probes[1].get("peak", 0) / 1e6, tt / tf, verdict, "equal on every frame" if same else "DIFFER"),
                  flush=True)
    print("fused faster at every size: %s" % ("yes" if all(ahead) else "no"))


if __name__ == "__main__":
    main()
