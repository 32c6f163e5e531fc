"""Mint the online tracker's known answers with the REFERENCE IDOL_Tracker (build container only).

    UNINEXT_REFERENCE=<reference checkout> python tests/golden/make_tracker_golden.py

Takes, with `ast` at generation time, `IDOL_Tracker`, `mask_iou` and `mask_nms` (projects/UNINEXT/uninext/models/tracker.py:17-298)
out of the reference checkout and runs them on the CPU in fp32 over the sequences of tests/tracker_cases.py.  Nothing of the
reference's text is stored.  tests/golden/tracker/<case>.npz holds, per frame, the ids, the indices and the number of detections
the pre-NMS kept, and the final `memo` (the embeddings and the rings as row sums: a bank of 65 rings would not fit a fixture);
the inputs are rebuilt from the case's seed.  tests/golden/tracker/signature.json holds the names and defaults of the
constructor's arguments and the names of match's.

The generator ASSERTS that every case keeps the float64 margin of tests/tracker_cases.py on every frame, that the float64
restatement (tests/tracker_ref.py) gives the reference's integers, and that the cases reach the edges they are named for."""
import ast
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tracker_cases as C  # noqa: E402
import tracker_ref  # noqa: E402

TRACKER = os.path.join(os.environ["UNINEXT_REFERENCE"], "projects/UNINEXT/uninext/models/tracker.py")
MAX_BYTES = 64 * 1024

# what the set of cases has to reach (events of tests/tracker_ref.py)
REACHED = {
    "bookkeeping": {"reappeared_after_2", "reappeared_after_3", "expired", "ring_wrapped", "memory_emptied"},
    "decisions": {"column_zeroed_under_a_rival", "backdrop", "backdrop_first", "left_unselected"},
    "frame_weight": {"frame_weight", "frame_weight_changed_winner"},
}


def load_reference():
    tree = ast.parse(open(TRACKER).read())
    picked = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in ("mask_iou", "mask_nms", "IDOL_Tracker")]
    assert len(picked) == 3
    ns = {"torch": torch, "F": F}
    exec(compile(ast.Module(body=picked, type_ignores=[]), TRACKER, "exec"), ns)
    return ns["IDOL_Tracker"]


def signature(cls):
    init = inspect.signature(cls.__init__).parameters
    return {"init": [[k, v.default] for k, v in init.items() if k != "self"],
            "match": [k for k in inspect.signature(cls.match).parameters if k != "self"]}


def main():
    cls = load_reference()
    os.makedirs(C.GOLDEN, exist_ok=True)
    with open(os.path.join(C.GOLDEN, "signature.json"), "w") as f:
        json.dump(signature(cls), f, indent=1)
    warnings.simplefilter("ignore")            # torch.range is deprecated
    for name, (_, D, seed, kwargs) in C.CASES.items():
        ref64 = tracker_ref.run(name, C)
        assert min(ref64["margins"]) >= C.MARGIN, (name, "reseed: margins", ref64["margins"])
        assert REACHED.get(name, set()) <= ref64["events"], (name, ref64["events"])
        tracker = cls(**kwargs)
        save = {"seed": np.int64(seed), "frames": np.int64(len(C.frames(name)))}
        kept = []
        for t, fr in enumerate(C.frames(name)):
            _, _, ids, indices = tracker.match(fr["bboxes"].clone(), fr["labels"].clone(), fr["masks"].clone(), fr["embeds"].clone(),
                                               fr["frame_id"], list(fr["indices"]))
            assert (ids.tolist(), indices, len(indices)) == ref64["frames"][t], (name, t)
            save["%d.ids" % t] = ids.numpy().astype(np.int64)
            save["%d.indices" % t] = np.asarray(indices, dtype=np.int64)
            kept.append(len(indices))
        save["kept"] = np.asarray(kept, dtype=np.int64)
        memo = C.memo_arrays(tracker.memo)
        C.assert_memo_close(memo, ref64["memo"], name)
        for key in ("embeds", "long_embeds"):
            memo[key + "_rowsum"] = memo.pop(key).sum(1)
        for key, value in memo.items():
            save["memo." + key] = value
        path = os.path.join(C.GOLDEN, "%s.npz" % name)
        np.savez_compressed(path, **save)
        print("%-28s %d frames, kept %s, margin %.2e, %d tracklets at the end, %d bytes"
              % (name, len(kept), kept, min(ref64["margins"]), len(memo["ids"]), os.path.getsize(path)))
        assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    main()
