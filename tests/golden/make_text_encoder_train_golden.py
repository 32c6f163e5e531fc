"""Mint golden GRADIENTS for the text encoder with the installed `transformers.BertModel` driven by the REFERENCE's own
`BertEncoder.forward` (build container only: needs `transformers` and the reference checkout, UNINEXT_REFERENCE).

    python tests/golden/make_text_encoder_train_golden.py

As tests/golden/make_text_encoder_golden.py: `transformers.BertModel(config, add_pooling_layer=False)` on
tests/text_encoder_cases.py's small config, float64, CPU, eager attention, EVAL mode (no dropout), loaded strictly from the seeded
dyadic parameters; the reference's `BertEncoder` class with its `__init__` bypassed, its `forward` run as it is.  The loss is
sum(ret["hidden"] * U) for tests/text_encoder_train_cases.py's seeded dyadic U, and autograd runs through transformers' own
modules.

Cases: `padded`, `one_token`, and `parallel_det` -- the `padded` inputs with parallel_det on and task="detection", so the
reference's forward builds its [B, T, T] float mask itself.  transformers 5.x refuses that float mask
(masking_utils: "bitwise_and_cpu" not implemented for 'Float') and reads a 3-D bool mask as a padding mask; the `model` the
reference calls is therefore a thin function that extends the reference's mask the way transformers 4.x, which the reference
was written against, did (get_extended_attention_mask: (1 - mask[:, None]) * finfo.min, [B, 1, T, T]) -- a 4-D mask is what
5.x adds to the scores as it is.  The mask's values, built by the reference's loop, are untouched and recorded.

Each tests/golden/text_encoder_train/<case>.npz holds only data: the inputs and U, the last hidden state, the gradient of the
embeddings' output, of every bias and LayerNorm parameter and of layer 0's q / k / v weights (under "grad/<state-dict key>"),
and the digest of the parameters -- no weights."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import text_encoder_cases as C  # noqa: E402
import text_encoder_train_cases as TC  # noqa: E402

REF = os.environ.get("UNINEXT_REFERENCE", "/root/reference")
BERT = os.path.join(REF, "projects/UNINEXT/uninext/models/deformable_detr/bert_model.py")


def reference_encoder(hf, parallel_det, seen):
    spec = importlib.util.spec_from_file_location("reference_bert_model", BERT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    enc = mod.BertEncoder.__new__(mod.BertEncoder)
    torch.nn.Module.__init__(enc)
    enc.parallel_det = parallel_det

    def model(**kw):
        m = kw["attention_mask"]
        if m.dim() == 3:                                              # the reference's float [B, T, T] mask, extended as 4.x did
            seen["mask"] = m.clone()
            kw["attention_mask"] = (1.0 - m.double()[:, None, :, :]) * torch.finfo(torch.float64).min
        out = hf(**kw)
        seen["hidden"] = out.hidden_states
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
    os.makedirs(TC.HERE, exist_ok=True)
    U = TC.loss_weights()
    for name, (inputs, det) in TC.FIXTURES.items():
        ids, mask, _ = C.make_inputs(inputs)
        hf.zero_grad(set_to_none=True)
        seen = {}
        ret = reference_encoder(hf, det, seen)({"input_ids": ids, "attention_mask": mask}, task="detection" if det else None)
        hidden = seen["hidden"]
        assert len(hidden) == C.CONFIG["num_hidden_layers"] + 1 and torch.equal(hidden[-1], ret["hidden"])
        hidden[0].retain_grad()
        (ret["hidden"] * U).sum().backward()
        out = {"input_ids": ids.numpy(), "attention_mask": mask.numpy(), "U": U.numpy(), "hidden": ret["hidden"].detach().numpy(),
               "grad_embeddings_output": hidden[0].grad.numpy(), "digest": np.float64(C.digest(state)),
               "transformers": np.array(transformers.__version__)}
        if det:
            out["core_mask"] = seen["mask"].numpy().astype(np.uint8)
        for key, prm in hf.state_dict(keep_vars=True).items():
            if TC.recorded(key) and prm.requires_grad:
                out["grad/" + key] = prm.grad.numpy()
        np.savez_compressed(os.path.join(TC.HERE, name + ".npz"), **out)
        print(name, os.path.getsize(os.path.join(TC.HERE, name + ".npz")), "bytes", len(out), "entries")


if __name__ == "__main__":
    main()
