"""Mint the fixtures of tests/test_reference_on_top_cpu.py and tests/test_reference_entry_points_cpu.py with the
REFERENCE's own code (build container only: the tests themselves read nothing outside the repository).

    UNINEXT_REFERENCE=<reference checkout> python tests/golden/make_reference_glue_golden.py

Everything lands in tests/golden/reference_glue/ and is data only -- no reference source is stored.  Parameters and inputs
are not stored either: module_case() / enclayer_case() draw them (float32-exact values) from seeded CPU generators, the tests
draw them again and check the stored `digest`; the reference computes on them in float64 and its results are stored in
float32:
  binding.json       the module that ops/functions/ms_deform_attn_func.py imports as MSDA and the MSDA functions it calls;
  testpy.npz         ops/test.py:21-36's inputs and `ms_deform_attn_core_pytorch`'s output on them, float64 and float32;
  module.npz         the reference's MSDeformAttn(256, 4, 8, 4) of ops/modules/ms_deform_attn.py in float64 on its own CPU path
                     (`ms_deform_attn_core_pytorch`): encoder-form output, the gradients of out.sum() with respect to the
                     query and -- in factored form, see module() -- to every parameter, decoder-form output;
  configs.json       what detectron2.config.get_cfg() + uninext/config.py::add_uninext_config + merge_from_file make of the
                     two R50 yamls, and whether the frozen config refuses an assignment;
  enclayer_d512.npz  the reference's DeformableTransformerEncoderLayer (deformable_transformer_dino.py:330-370, d_ffn 512) in
                     float64: output.
`detectron2.config` imports fvcore / yacs / iopath / omegaconf / termcolor; where they are not installed the config pass
puts THROW-AWAY stand-ins for exactly those third-party modules in place while it runs.
"""
import ast
import contextlib
import copy
import importlib
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_glue")
REF = os.environ.get("UNINEXT_REFERENCE", "")     # a checkout of the reference repository
UX = os.path.join(REF, "projects/UNINEXT/uninext")
OPS = os.path.join(UX, "models/deformable_detr/ops")
R50_YAMLS = ("image_joint_r50.yaml", "obj365v2_32g_r50.yaml")


# ---- throw-away stand-ins for the missing third-party modules -------------------------------------------------------
class _CfgNode(dict):
    """The subset of yacs.config.CfgNode (+ fvcore's load_yaml_with_base) that detectron2.config uses."""
    IMMUTABLE, NEW_ALLOWED = "__immutable__", "__new_allowed__"

    def __init__(self, init_dict=None, key_list=None, new_allowed=False):
        super().__init__()
        self.__dict__[_CfgNode.IMMUTABLE] = False
        self.__dict__[_CfgNode.NEW_ALLOWED] = new_allowed
        for k, v in (init_dict or {}).items():
            self[k] = type(self)(v) if isinstance(v, dict) and not isinstance(v, _CfgNode) else v

    def __getattr__(self, name):
        if name in self:
            return self[name]
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if self.is_frozen():
            raise AttributeError("Attempted to set {} to {}, but CfgNode is immutable".format(name, value))
        self[name] = value

    def is_frozen(self):
        return self.__dict__[_CfgNode.IMMUTABLE]

    def _set_frozen(self, flag):
        self.__dict__[_CfgNode.IMMUTABLE] = flag
        for v in self.values():
            if isinstance(v, _CfgNode):
                v._set_frozen(flag)

    def freeze(self):
        self._set_frozen(True)

    def defrost(self):
        self._set_frozen(False)

    def clone(self):
        return copy.deepcopy(self)

    @staticmethod
    def _decode(v):
        if isinstance(v, dict):
            return v
        if not isinstance(v, str):
            return v
        try:
            return ast.literal_eval(v)
        except (ValueError, SyntaxError):
            return v

    @classmethod
    def load_yaml_with_base(cls, filename, allow_unsafe=False):
        import yaml
        with open(filename) as f:
            cfg = yaml.safe_load(f)
        base = cfg.pop("_BASE_", None)
        if base is not None:
            if not os.path.isabs(base):
                base = os.path.join(os.path.dirname(filename), base)
            merged = cls.load_yaml_with_base(base, allow_unsafe)

            def rec(a, b):
                for k, v in a.items():
                    if isinstance(v, dict) and isinstance(b.get(k), dict):
                        rec(v, b[k])
                    else:
                        b[k] = v
            rec(cfg, merged)
            return merged
        return cfg

    def merge_from_other_cfg(self, other):
        def rec(a, b, path):
            for k, v in a.items():
                v = _CfgNode._decode(v)
                if k not in b:
                    if b.__dict__[_CfgNode.NEW_ALLOWED]:
                        b[k] = v
                        continue
                    raise KeyError("Non-existent config key: {}".format(".".join(path + [k])))
                if isinstance(b[k], _CfgNode):
                    rec(v, b[k], path + [k])
                else:
                    old = b[k]
                    if isinstance(old, tuple) and isinstance(v, list):
                        v = tuple(v)
                    elif isinstance(old, list) and isinstance(v, tuple):
                        v = list(v)
                    elif old is not None and v is not None and type(old) is not type(v) and not (
                            isinstance(old, (int, float)) and isinstance(v, (int, float))):
                        raise ValueError("Type mismatch for {}: {} vs {}".format(".".join(path + [k]), type(old), type(v)))
                    b[k] = v
        rec(other, self, [])

    def merge_from_list(self, cfg_list):
        for full_key, v in zip(cfg_list[0::2], cfg_list[1::2]):
            d = self
            keys = full_key.split(".")
            for k in keys[:-1]:
                d = d[k]
            d[keys[-1]] = _CfgNode._decode(v)


class _Registry:
    def __init__(self, name):
        self._name, self._obj_map = name, {}

    def register(self, obj=None):
        if obj is None:
            def deco(o):
                self._obj_map[o.__name__] = o
                return o
            return deco
        self._obj_map[obj.__name__] = obj

    def get(self, name):
        if name not in self._obj_map:
            raise KeyError("No object named '{}' found in '{}' registry!".format(name, self._name))
        return self._obj_map[name]

    def __contains__(self, name):
        return name in self._obj_map


class _PathManager:
    def open(self, path, mode="r", **kw):
        return open(path, mode)

    def isfile(self, path):
        return os.path.isfile(path)

    def get_local_path(self, path, **kw):
        return path

    def register_handler(self, handler, **kw):
        pass


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    return m


@contextlib.contextmanager
def d2():
    """sys.modules / sys.path with the stand-ins and the reference on them; restored afterwards."""
    saved_modules, saved_path = dict(sys.modules), list(sys.path)
    for k in [k for k in sys.modules if k.split(".")[0] in ("detectron2", "fvcore", "iopath", "omegaconf", "termcolor", "refops")]:
        del sys.modules[k]
    ph = type("PathHandler", (), {})
    stubs = {
        "fvcore": _mod("fvcore", __version__="0.1.5"), "fvcore.common": _mod("fvcore.common"),
        "fvcore.common.config": _mod("fvcore.common.config", CfgNode=_CfgNode),
        "fvcore.common.registry": _mod("fvcore.common.registry", Registry=_Registry),
        "iopath": _mod("iopath"), "iopath.common": _mod("iopath.common"),
        "iopath.common.file_io": _mod("iopath.common.file_io", PathManager=_PathManager, PathHandler=ph,
                                      HTTPURLHandler=type("HTTPURLHandler", (ph,), {}),
                                      OneDrivePathHandler=type("OneDrivePathHandler", (ph,), {})),
        "omegaconf": _mod("omegaconf", DictConfig=type("DictConfig", (), {}), ListConfig=type("ListConfig", (), {}),
                          OmegaConf=type("OmegaConf", (), {}), SCMode=type("SCMode", (), {})),
        "termcolor": _mod("termcolor", colored=lambda s, *a, **k: s),
    }
    sys.modules.update(stubs)
    sys.path.insert(0, REF)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            yield importlib.import_module("detectron2.config")
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_modules:
                del sys.modules[k]
        sys.modules.update(saved_modules)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def binding():
    """The name ms_deform_attn_func.py imports as MSDA (:18) and the MSDA attributes it calls (:26, :36)."""
    tree = ast.parse(open(os.path.join(OPS, "functions/ms_deform_attn_func.py")).read())
    module = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names if a.asname == "MSDA"]
    calls = sorted({n.attr for n in ast.walk(tree)
                    if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "MSDA"})
    assert len(module) == 1 and calls
    rec = {"module": module[0], "functions": calls}
    with open(os.path.join(OUT, "binding.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("binding", rec)


def reference_core():
    sys.modules.setdefault("MultiScaleDeformableAttention", types.ModuleType("MultiScaleDeformableAttention"))
    return _load(os.path.join(OPS, "functions/ms_deform_attn_func.py"), "_ref_func").ms_deform_attn_core_pytorch


def testpy():
    """ops/test.py:21-36 and its forward check's `ms_deform_attn_core_pytorch` output, float64 and float32."""
    core = reference_core()
    N, M, D = 1, 2, 2
    Lq, L, P = 2, 2, 2
    shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    S = sum((H * W).item() for H, W in shapes)
    torch.manual_seed(3)
    value = torch.rand(N, S, M, D) * 0.01
    loc = torch.rand(N, Lq, M, L, P, 2)
    attn = torch.rand(N, Lq, M, L, P) + 1e-5
    attn /= attn.sum(-1, keepdim=True).sum(-2, keepdim=True)
    arrays = {"shapes": shapes.numpy(), "lsi": lsi.numpy()}
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        v, lo, a = value.to(dtype), loc.to(dtype), attn.to(dtype)
        arrays.update({"value_" + tag: v.numpy(), "loc_" + tag: lo.numpy(), "attn_" + tag: a.numpy(),
                       "want_" + tag: core(v, shapes, lo, a).numpy()})
    np.savez_compressed(os.path.join(OUT, "testpy.npz"), **arrays)
    print("testpy", {k: v.shape for k, v in arrays.items()})


def level_tensors(levels):
    shapes = torch.as_tensor(levels, dtype=torch.long)
    return shapes, torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def encoder_reference_points(levels):
    """Cell centres of every level, normalised (the reference encoder's get_reference_points, valid ratios 1)."""
    pts = []
    for h, w in levels:
        y, x = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=torch.float64),
                              torch.linspace(0.5, w - 0.5, w, dtype=torch.float64), indexing="ij")
        pts.append(torch.stack((x.reshape(-1) / w, y.reshape(-1) / h), -1))
    return torch.cat(pts, 0)


def _draw(g, *shape, scale=1.0):
    """float64 values that float32 holds exactly, from the seeded CPU generator `g`."""
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float().double()


def _offset_bias_pattern(heads, levels, points):
    """MSDeformAttn's initial sampling_offsets bias (ops/modules/ms_deform_attn.py:_reset_parameters): one direction per
    head, scaled by the point index."""
    theta = torch.arange(heads, dtype=torch.float64) * (2.0 * torch.pi / heads)
    grid = torch.stack([theta.cos(), theta.sin()], -1)
    grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(heads, 1, 1, 2).repeat(1, levels, points, 1)
    return (grid * torch.arange(1, points + 1, dtype=torch.float64).view(1, 1, points, 1)).reshape(-1)


def _msda_params(g, d_model=256, heads=8, levels=4, points=4, prefix=""):
    p = {}

    def lin(name, o, i, wstd):
        p[prefix + name + ".weight"] = _draw(g, o, i, scale=wstd)
        p[prefix + name + ".bias"] = _draw(g, o, scale=0.1)
    lin("sampling_offsets", heads * levels * points * 2, d_model, 0.02)
    p[prefix + "sampling_offsets.bias"] = (p[prefix + "sampling_offsets.bias"]
                                           + _offset_bias_pattern(heads, levels, points)).float().double()
    lin("attention_weights", heads * levels * points, d_model, 0.05)
    lin("value_proj", d_model, d_model, 1.0 / 16)
    lin("output_proj", d_model, d_model, 1.0 / 16)
    return p


def _digest(tensors):
    return float(sum(float(t.double().abs().sum()) for t in tensors))


MODULE_LEVELS = ((4, 6), (2, 3), (1, 2), (1, 1))
MODULE_LINEARS = ("sampling_offsets", "attention_weights", "value_proj", "output_proj")


def module_case(dtype=torch.float64):
    """Parameters and inputs of the MSDeformAttn(256, 4, 8, 4) fixture, drawn from a seeded CPU generator (shared by the test:
    only the reference's results are stored, pinned to these draws by `digest`)."""
    g = torch.Generator().manual_seed(11)
    params = _msda_params(g)
    S = sum(h * w for h, w in MODULE_LEVELS)
    src = _draw(g, 2, S, 256)
    ref4 = (torch.rand(2, 11, 4, 4, generator=g, dtype=torch.float64) * 0.5 + 0.25).float().double()
    q4 = _draw(g, 2, 11, 256)
    digest = _digest(list(params.values()) + [src, ref4, q4])
    shapes, lsi = level_tensors(MODULE_LEVELS)
    refpts = encoder_reference_points(MODULE_LEVELS)[None, :, None, :].expand(2, S, 4, 2).contiguous()
    mask = torch.zeros(2, S, dtype=torch.bool)
    mask[0, :7] = True
    to = lambda t: t.to(dtype)
    return dict(params={k: to(v) for k, v in params.items()}, src=to(src), refpts=to(refpts), shapes=shapes, lsi=lsi, mask=mask,
                ref4=to(ref4), query4=to(q4), digest=digest)


ENCLAYER_LEVELS = ((9, 12), (5, 6), (3, 3), (2, 2))


def enclayer_case(dtype=torch.float64):
    """Parameters and inputs of the DeformableTransformerEncoderLayer(d_ffn 512) fixture, drawn like module_case."""
    g = torch.Generator().manual_seed(4)
    params = _msda_params(g, prefix="self_attn.")
    params["linear1.weight"], params["linear1.bias"] = _draw(g, 512, 256, scale=1.0 / 16), _draw(g, 512, scale=0.1)
    params["linear2.weight"], params["linear2.bias"] = _draw(g, 256, 512, scale=1.0 / 23), _draw(g, 256, scale=0.1)
    for n in ("norm1", "norm2"):
        params[n + ".weight"] = (1.0 + _draw(g, 256, scale=0.1)).float().double()
        params[n + ".bias"] = _draw(g, 256, scale=0.1)
    S = sum(h * w for h, w in ENCLAYER_LEVELS)
    src, pos = _draw(g, 2, S, 256), _draw(g, 2, S, 256, scale=0.3)
    digest = _digest(list(params.values()) + [src, pos])
    shapes, lsi = level_tensors(ENCLAYER_LEVELS)
    ref = encoder_reference_points(ENCLAYER_LEVELS)[None, :, None, :].expand(2, S, 4, 2).contiguous()
    mask = torch.zeros(2, S, dtype=torch.bool)
    mask[1, -9:] = True
    to = lambda t: t.to(dtype)
    return dict(params={k: to(v) for k, v in params.items()}, src=to(src), pos=to(pos), ref=to(ref), shapes=shapes, lsi=lsi,
                mask=mask, digest=digest)


def f32(t):
    return t.detach().numpy().astype(np.float32)


def module():
    """The reference module in float64 on its own CPU path.  Gradients of out.sum(): the query's whole; those of every Linear
    y = x W^T + b in factored form -- dy (the gradient at the layer's output) and, for output_proj, whose input is internal,
    x -- from which dW = dy^T x and db = sum(dy) follow exactly (the other layers' x is the query or the input, both inputs)."""
    sys.path.insert(0, HERE)
    import make_encoder_layer_golden as mel
    mel.load_reference_layer()                         # the reference's ms_deform_attn.py on its own CPU path
    cls = sys.modules["refops.modules.ms_deform_attn"].MSDeformAttn
    c = module_case()
    theirs = cls(256, 4, 8, 4).double()
    theirs.load_state_dict(c["params"])
    src, refpts, shapes, lsi, mask = c["src"], c["refpts"], c["shapes"], c["lsi"], c["mask"]
    caught, handles = {}, []
    for name in MODULE_LINEARS:
        def fwd(m, inp, out, name=name):
            caught["x:" + name] = inp[0].detach()
            out.register_hook(lambda gy, name=name: caught.__setitem__("dy:" + name, gy.detach()))
        handles.append(getattr(theirs, name).register_forward_hook(fwd))
    q = src.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = theirs(q, refpts, src, shapes, lsi, mask)
        out.sum().backward()
        for h in handles:
            h.remove()
        with torch.no_grad():
            out4 = theirs(c["query4"], c["ref4"], src, shapes, lsi, None)
    for name in MODULE_LINEARS:                        # the factored form reproduces the reference's own weight gradients
        lin = getattr(theirs, name)
        dy, x = caught["dy:" + name], caught["x:" + name]
        assert torch.allclose(dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1]), lin.weight.grad, rtol=1e-10, atol=1e-12)
    assert torch.equal(caught["x:value_proj"], src) and torch.equal(caught["x:sampling_offsets"], q.detach())
    arrays = {"out": f32(out), "grad_query": f32(q.grad), "out4": f32(out4), "digest": np.float64(c["digest"]),
              "x:output_proj": f32(caught["x:output_proj"])}
    arrays.update({"dy:" + n: f32(caught["dy:" + n]) for n in MODULE_LINEARS})
    np.savez_compressed(os.path.join(OUT, "module.npz"), **arrays)
    print("module", tuple(out.shape), "scale", float(out.abs().max()), {k: v.shape for k, v in arrays.items()})


def enclayer():
    sys.path.insert(0, HERE)
    import make_encoder_layer_golden as mel
    cls = mel.load_reference_layer()
    c = enclayer_case()
    theirs = cls(d_model=256, d_ffn=512, dropout=0.0, n_levels=4, n_heads=8, n_points=4).double().eval()
    theirs.load_state_dict(c["params"])
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        out = theirs(c["src"], c["pos"], c["ref"], c["shapes"], c["lsi"], c["mask"])
    np.savez_compressed(os.path.join(OUT, "enclayer_d512.npz"), out=f32(out), digest=np.float64(c["digest"]))
    print("enclayer_d512", tuple(out.shape), "scale", float(out.abs().max()))


def configs():
    rec = {}
    with d2() as config:
        add_uninext_config = _load(os.path.join(UX, "config.py"), "ref_uninext_config").add_uninext_config
        for name in R50_YAMLS:
            cfg = config.get_cfg()
            add_uninext_config(cfg)
            cfg.merge_from_file(os.path.join(REF, "projects/UNINEXT/configs", name))
            cfg.freeze()
            dd = cfg.MODEL.DDETRS
            try:
                cfg.MODEL.OTA = False
                frozen = False
            except AttributeError:
                frozen = True
            rec[name] = {"MODEL.META_ARCHITECTURE": cfg.MODEL.META_ARCHITECTURE, "MODEL.OTA": cfg.MODEL.OTA,
                         "MODEL.DDETRS": {k: dd[k] for k in ("NUM_OBJECT_QUERIES", "HIDDEN_DIM", "NHEADS", "NUM_FEATURE_LEVELS",
                                                             "ENC_N_POINTS", "DEC_N_POINTS", "ENC_LAYERS", "DEC_LAYERS",
                                                             "DIM_FEEDFORWARD")},
                         "frozen_refuses_assignment": frozen}
    with open(os.path.join(OUT, "configs.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("configs", rec)


if __name__ == "__main__":
    if not os.path.isdir(os.path.join(REF, "detectron2")):
        raise SystemExit("set UNINEXT_REFERENCE to a checkout of the reference repository")
    os.makedirs(OUT, exist_ok=True)
    binding()
    testpy()
    module()
    enclayer()
    configs()
