"""Mint golden vectors for the text encoder with the installed `transformers.BertModel` driven by the REFERENCE's own
`BertEncoder.forward` (build container only: needs `transformers` and the reference checkout, UNINEXT_REFERENCE).

    python tests/golden/make_text_encoder_golden.py

`transformers.BertModel(config, add_pooling_layer=False)` on tests/text_encoder_cases.py's small config, float64, CPU, eager
attention, loaded strictly from the seeded dyadic parameters.  The reference's `BertEncoder` class is imported and its
`__init__` bypassed (it wants a checkpoint directory); its `forward` runs as it is on {"input_ids", "attention_mask"}.  The
`model` it calls is a thin function around the transformers model that records every hidden state (the reference keeps only
the last) and, for the `type_ids` case, passes the token type ids that the reference's forward has no argument for.

Each tests/golden/text_encoder/<case>.npz holds the inputs, every hidden state, the reference's returned "hidden" and "masks",
and the digest of the parameters -- no weights.  state_dict_keys.json holds the transformers model's state-dict keys and shapes.

The PARALLEL_DET case is NOT minted: the reference builds a float [B, T, T] mask, and transformers 5.x refuses it
(masking_utils.sdpa_mask: "bitwise_and_cpu" not implemented for 'Float').  That route rests on the float64 restatement
(tests/text_encoder_ref.py) alone, which the fixtures here pin on the 2-D masks."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import text_encoder_cases as C  # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
BERT = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/bert_model.py")


def reference_encoder(hf, token_type_ids, seen):
    spec = importlib.util.spec_from_file_location("reference_bert_model", BERT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    enc = mod.BertEncoder.__new__(mod.BertEncoder)
    torch.nn.Module.__init__(enc)
    enc.parallel_det = False

    def model(**kw):
        if token_type_ids is not None:
            kw["token_type_ids"] = token_type_ids
        out = hf(**kw)
        seen.append(out.hidden_states)
        return out
    enc.model = model
    return enc


def main():
    import transformers
    cfg = transformers.BertConfig(hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, **C.CONFIG)
    cfg._attn_implementation = "eager"
    hf = transformers.BertModel(cfg, add_pooling_layer=False).double().eval()
    state = C.state_dict()
    missing = hf.load_state_dict(state, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    os.makedirs(C.HERE, exist_ok=True)
    with open(os.path.join(C.HERE, "state_dict_keys.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in hf.state_dict().items()}, f, indent=1)
    for name in C.FIXTURES:
        ids, mask, tt = C.make_inputs(name)
        seen = []
        with torch.no_grad():
            ret = reference_encoder(hf, tt, seen)({"input_ids": ids, "attention_mask": mask})
        hidden = seen[0]
        assert len(hidden) == C.CONFIG["num_hidden_layers"] + 1 and torch.equal(hidden[-1], ret["hidden"])
        out = {"input_ids": ids.numpy(), "attention_mask": mask.numpy(), "masks": ret["masks"].numpy(), "hidden": ret["hidden"].numpy(),
               "digest": np.float64(C.digest(state)), "transformers": np.array(transformers.__version__)}
        if tt is not None:
            out["token_type_ids"] = tt.numpy()
        for n, h in enumerate(hidden):
            out["hidden_%d" % n] = h.numpy()
        np.savez_compressed(os.path.join(C.HERE, name + ".npz"), **out)
        print(name, {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
