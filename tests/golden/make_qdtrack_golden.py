"""Mint the QuasiDense tracker's known answers with the REFERENCE QuasiDenseEmbedTracker (build container only).

    UNINEXT_REFERENCE=<reference checkout> python tests/golden/make_qdtrack_golden.py

Takes, with `ast` at generation time, `QuasiDenseEmbedTracker` (projects/UNINEXT/uninext/models/tracker.py:304-503) and
`bbox_overlaps` with `fp16_clamp` (projects/UNINEXT/uninext/util/mmcv_utils.py) out of the reference checkout and runs them on the
CPU in fp32 over the sequences of tests/qdtrack_cases.py.  Nothing of the reference's text is stored.
tests/golden/qdtrack/<case>.npz holds, per frame, the ids, the indices and the number of detections the pre-NMS kept, the final
`memo` (the embeddings as row sums) with the tracklets' last_frame / acc_frame and the backdrop frames' rows, and the reference's
bbox_overlaps of the score-sorted boxes of the frames qdtrack_cases.IOU_FRAMES; the inputs are rebuilt from the case's seed.
tests/golden/qdtrack/signature.json holds the names and defaults of the constructor's arguments and the names of match's.

The generator ASSERTS that every case keeps the float64 margin of tests/tracker_cases.py on every frame, that the float64
restatement (tests/qdtrack_ref.py) gives the reference's integers, and that the cases reach the edges they are named for."""
import ast
import inspect
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import qdtrack_cases as C  # noqa: E402
import qdtrack_ref  # noqa: E402

UNINEXT = os.path.join(os.environ["UNINEXT_REFERENCE"], "projects/UNINEXT/uninext")
MAX_BYTES = 64 * 1024

# what the set of cases has to reach (events of tests/qdtrack_ref.py)
REACHED = {
    "bookkeeping": {"reappeared_after_2", "reappeared_after_3", "expired", "memory_emptied", "no_tracklets_while_backdrops_exist",
                    "starts_no_tracklet_while_backdrops_exist"},
    "decisions": {"backdrop_best_then_new_tracklet", "minus_two", "column_zeroed_under_a_rival", "all_but_the_first_dropped",
                  "dropped_by_dropped_rows_alone", "backdrop_filtered"},
    "cats_on": {"cross_class_best_column"},
    "cats_off": {"cross_class_best_column"},
    "ring2": {"best_column_is_a_backdrop"},
}


def pick(path, names):
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(picked) == len(names), (path, names)
    return ast.Module(body=picked, type_ignores=[]), path


def load_reference():
    ns = {"torch": torch, "F": F}
    for path, names in ((os.path.join(UNINEXT, "util/mmcv_utils.py"), ("fp16_clamp", "bbox_overlaps")),
                        (os.path.join(UNINEXT, "models/tracker.py"), ("QuasiDenseEmbedTracker",))):
        exec(compile(*pick(path, names), "exec"), ns)
    return ns["QuasiDenseEmbedTracker"], ns["bbox_overlaps"]


def signature(cls):
    init = inspect.signature(cls.__init__).parameters
    return {"init": [[k, v.default] for k, v in init.items() if k != "self"],
            "match": [k for k in inspect.signature(cls.match).parameters if k != "self"]}


class Shim:
    """The reference's tracker under the names tests/qdtrack_cases.py: memo_arrays reads"""

    def __init__(self, tracker):
        self.tracklets, self.backdrops, self.tracker = tracker.tracklets, tracker.backdrops, tracker

    @property
    def memo(self):
        return self.tracker.memo


def main():
    cls, overlaps = load_reference()
    os.makedirs(C.GOLDEN, exist_ok=True)
    with open(os.path.join(C.GOLDEN, "signature.json"), "w") as f:
        json.dump(signature(cls), f, indent=1)
    for name, (_, D, seed, kwargs) in C.CASES.items():
        ref64 = qdtrack_ref.run(name, C)
        assert min(ref64["margins"]) >= C.MARGIN, (name, "reseed: margins", ref64["margins"])
        assert REACHED.get(name, set()) <= ref64["events"], (name, ref64["events"])
        tracker = cls(**kwargs)
        save = {"seed": np.int64(seed), "frames": np.int64(len(C.frames(name)))}
        kept = []
        for t, fr in enumerate(C.frames(name)):
            _, _, ids, indices = tracker.match(fr["bboxes"].clone(), fr["labels"].clone(), fr["embeds"].clone(), fr["frame_id"],
                                               list(fr["indices"]))
            assert (ids.tolist(), indices, len(indices)) == ref64["frames"][t], (name, t)
            save["%d.ids" % t] = ids.numpy().astype(np.int64)
            save["%d.indices" % t] = np.asarray(indices, dtype=np.int64)
            kept.append(len(indices))
            if t in C.IOU_FRAMES:
                boxes = fr["bboxes"][fr["bboxes"][:, -1].sort(descending=True)[1], :-1]
                iou = overlaps(boxes, boxes).numpy()
                assert iou.dtype == np.float32 and np.abs(iou - ref64["ious"][t]).max() <= 1e-6
                save["iou.%d" % t] = iou
        save["kept"] = np.asarray(kept, dtype=np.int64)
        memo = C.memo_arrays(Shim(tracker))
        C.assert_memo_close(memo, ref64["memo"], name)
        for key, value in C.with_rowsums(memo).items():
            save["memo." + key] = value
        path = os.path.join(C.GOLDEN, "%s.npz" % name)
        np.savez_compressed(path, **save)
        print("%-16s %d frames, kept %s, margin %.2e, %d tracklets and %s backdrops at the end, %d bytes"
              % (name, len(kept), kept, min(ref64["margins"]), len(memo["last_frame"]), memo["backdrop_rows"].tolist(), os.path.getsize(path)))
        assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main()
