"""Shared by tests/golden/make_text_encoder_train_golden.py, tests/test_text_encoder_train_cpu.py and
tests/test_text_encoder_train_gpu.py: the training route of the text encoder's attention core (include/dynmask_hip.h:
bert_hip_self_attention_train_f32, bert_hip_self_attention_backward_f32, bert_hip_dropout_keep_u8).

  * `core`: the header's formulas with an explicit keep matrix, in torch on the CPU, float64 (the reference) or float32 (the
    composition whose own error the tests print beside the kernels').  A query that keeps no key follows the header: a zero row
    of `out` and of dq, nothing added to dk and dv.
  * `keep_matrix`: the numpy Philox mirror of tests/vlfuse_dropout_cases.py at the header's counter layout (side 0).
  * `model_grads`: the float64 restatement of the whole encoder (tests/text_encoder_ref.py's statements) with `core` inside as
    an autograd function, for the loss sum(hidden * U): every parameter's gradient.
  * `group_errors`: max abs error over the group's max abs, per group dq, dk, dv (and whatever else is handed in).
  * the fixtures under tests/golden/text_encoder_train/ and the loss weights U.

The bound is text_encoder_cases.TOL = 1e-4, the project's fp32 bound against float64."""
import math
import os

import numpy as np
import torch

import text_encoder_cases as C
import text_encoder_ref as R
import vlfuse_dropout_cases as DC

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_encoder_train")
TOL, TOL64 = C.TOL, C.TOL64
GROUPS = ("dq", "dk", "dv")
# name -> (the inputs of text_encoder_cases.make_inputs, through the reference's PARALLEL_DET mask)
FIXTURES = {"padded": ("padded", False), "one_token": ("one_token", False), "parallel_det": ("padded", True)}

seed_of, scale_of, threshold_of = DC.seed_of, DC.scale_of, DC.threshold_of


def keep_matrix(seed, p, BH, T):
    """[BH, T, T] bool indexed [bh, query, key]: counter (offset low, offset high, query, bh << 8 | key / 4), word key % 4,
    keep <=> word >= threshold -- the bi-attention core's side 0 with the query in the image token's place."""
    return DC.keep_masks(seed, p, BH, T, T)[0]


def loss_weights(name="text_encoder_train_U"):
    """U [B, T, hidden]: seeded dyadics; the loss of the fixtures is sum(last hidden state * U)."""
    g = torch.Generator().manual_seed(C.SEED + 100)
    return C.dyadic(torch.randn(C.B, C.T, C.CONFIG["hidden_size"], generator=g))


def kept(mask, B, T):
    """[B, 1 or T, T] bool from None, a [B, T] or a [B, T, T] keep mask"""
    if mask is None:
        return torch.ones(B, 1, T, dtype=torch.bool)
    m = torch.as_tensor(mask).cpu() != 0
    return m[:, None, :] if m.dim() == 2 else m


def core(q, k, v, heads, mask=None, g=None, keep=None, p=0.0, dt=torch.float64):
    """q, k, v (and g = grad_out) [B, T, heads * d]; mask a keep mask or None; keep [B * heads, T, T] (bool, 1 = kept) or None;
    p the dropout probability.  Returns out, lse [B * heads, T] and -- with g -- dq, dk, dv, all token-major, in `dt`."""
    q, k, v = (torch.as_tensor(t).cpu().to(dt) for t in (q, k, v))
    B, T, E = q.shape
    d = E // heads
    scale = d ** -0.5
    split = lambda t: t.reshape(B, T, heads, d).permute(0, 2, 1, 3)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, E)
    qs = split(q) * scale                                             # q is scaled first
    s = qs @ split(k).transpose(-1, -2)
    km = kept(mask, B, T)[:, None]                                    # [B, 1, 1 or T, T]
    s = torch.where(km, s, torch.full_like(s, -math.inf))
    lse = torch.logsumexp(s, -1, keepdim=True)                        # -inf for a query that keeps no key
    prob = torch.where(km, torch.exp(s - torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)), torch.zeros_like(s))
    c = float(scale_of(p)) if dt == torch.float64 else torch.tensor(scale_of(p))
    cm = torch.ones_like(s) if keep is None else torch.as_tensor(np.asarray(keep)).reshape(B, heads, T, T).to(dt) * c
    pd = cm * prob
    out = pd @ split(v)
    res = dict(out=merge(out), lse=lse.reshape(B * heads, T))
    if g is not None:
        gs = split(torch.as_tensor(g).cpu().to(dt))
        delta = (gs * out).sum(-1, keepdim=True)
        dp = cm * (gs @ split(v).transpose(-1, -2))
        ds = prob * (dp - delta)
        res.update(dq=merge(ds @ split(k)) * scale, dk=merge(ds.transpose(-1, -2) @ qs), dv=merge(pd.transpose(-1, -2) @ gs))
    return res


def group_errors(got, want, comp=None, names=GROUPS):
    """{name: (max abs error / the group's max abs, the same of the fp32 composition or None)}"""
    out = {}
    for n in names:
        w = torch.as_tensor(want[n]).double()
        unit = float(w.abs().max()) or 1.0
        err = float((torch.as_tensor(got[n]).detach().cpu().double() - w).abs().max()) / unit
        cerr = None if comp is None else float((torch.as_tensor(comp[n]).detach().cpu().double() - w).abs().max()) / unit
        out[n] = (err, cerr)
    return out


def report(who, errs):
    """Prints every figure and its ratio to the composition's own error; returns the largest figure."""
    for n, (err, cerr) in errs.items():
        ratio = "" if cerr is None else "  comp %.3e  ratio %s" % (cerr, "%.2f" % (err / cerr) if cerr > 0 else "inf" if err > 0 else "0")
        print("%-44s %-8s err %.3e%s" % (who, n, err, ratio))
    return max(e for e, _ in errs.values())


# ---- the whole encoder in float64 with `core` inside ---------------------------------------------------------------------
class _Core(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, mask, keep, p):
        ctx.save_for_backward(q, k, v)
        ctx.args = (heads, mask, keep, p)
        return core(q, k, v, heads, mask, None, keep, p)["out"]

    @staticmethod
    def backward(ctx, g):
        q, k, v = ctx.saved_tensors
        heads, mask, keep, p = ctx.args
        r = core(q, k, v, heads, mask, g, keep, p)
        return r["dq"], r["dk"], r["dv"], None, None, None, None


def _layer(p, pre, x, heads, mask, eps, keep, prob):
    lin = lambda name, t: t @ p[pre + name + ".weight"].T + p[pre + name + ".bias"]
    ctx = _Core.apply(lin("attention.self.query", x), lin("attention.self.key", x), lin("attention.self.value", x), heads, mask, keep, prob)
    x = R.layer_norm(lin("attention.output.dense", ctx) + x, p[pre + "attention.output.LayerNorm.weight"],
                     p[pre + "attention.output.LayerNorm.bias"], eps)
    y = lin("output.dense", R.gelu(lin("intermediate.dense", x)))
    return R.layer_norm(y + x, p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)


def model_grads(ids, mask, U, tt=None, keeps=None, p=0.0):
    """(hidden states, {parameter key: gradient}, gradient of the embeddings' output) of sum(last hidden * U) in float64, the
    attention core being `core`; keeps: per layer a [B * heads, T, T] keep matrix of the attention dropout, or None."""
    cfg = C.CONFIG
    params = {k: v.double().clone().requires_grad_(True) for k, v in C.state_dict().items()}
    x = R.embeddings(params, ids, tt, cfg["layer_norm_eps"])
    x.retain_grad()
    hidden = [x]
    for n in range(cfg["num_hidden_layers"]):
        x = _layer(params, "encoder.layer.%d." % n, x, cfg["num_attention_heads"], mask, cfg["layer_norm_eps"],
                   None if keeps is None else keeps[n], p)
        hidden.append(x)
    (x * U.double()).sum().backward()
    params["embeddings.word_embeddings.weight"].grad[0] = 0.0         # nn.Embedding(padding_idx=0): the padding row gets none
    return [h.detach() for h in hidden], {k: v.grad for k, v in params.items()}, hidden[0].grad


def module_grads(m, name, dtype=torch.float64, device="cpu"):
    """(last hidden state, {key: grad}, grad of the embeddings' output) of the project's BertModel `m` behind a BertEncoder on a
    fixture's inputs, for the loss sum(hidden * U)."""
    from uninext_amd import text_encoder as TE
    ids, mask, _ = fixture_inputs(name)
    enc = TE.BertEncoder(m, parallel_det=FIXTURES[name][1])
    m.zero_grad(set_to_none=True)
    seen = []

    def keep_grad(mod, args, out):
        out.retain_grad()
        seen.append(out)
    hook = m.embeddings.register_forward_hook(keep_grad)
    ret = enc({"input_ids": ids.to(device), "attention_mask": mask.to(device)}, task="detection")
    hook.remove()
    (ret["hidden"] * loss_weights().to(dtype).to(device)).sum().backward()
    return ret["hidden"].detach(), {k: p.grad for k, p in m.named_parameters()}, seen[0].grad


def recorded(key):
    """Whether the fixtures carry this parameter's gradient: every bias and LayerNorm parameter, layer 0's q / k / v weights."""
    return (key.endswith(".bias") or "LayerNorm" in key
            or (key.startswith("encoder.layer.0.attention.self.") and key.endswith(".weight")))


def param_err(key, got, want):
    """max abs error of a parameter's gradient over the gradient's max abs; `want` {key: gradient}.  A KEY BIAS is the exception:
    its gradient is zero in exact arithmetic (a softmax does not see a constant added to all scores of a row: sum_j ds[i, j] = 0),
    so what float64 leaves there is rounding noise and no unit; it is measured against the QUERY bias' gradient of its layer,
    which sums the same ds over the other index."""
    unit_key = key.replace(".key.bias", ".query.bias")
    w = torch.as_tensor(np.asarray(want[key])).double()
    unit = float(torch.as_tensor(np.asarray(want[unit_key])).double().abs().max()) or 1.0
    return float((torch.as_tensor(got).detach().cpu().double() - w).abs().max()) / unit


def load(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    return {k: z[k] for k in z.files}


def fixture_inputs(name):
    """(ids, the [B, T] mask, the mask the attention core sees) of a fixture"""
    inputs, det = FIXTURES[name]
    ids, mask, _ = C.make_inputs(inputs)
    return ids, mask, (R.parallel_det_mask(mask) if det else mask)
