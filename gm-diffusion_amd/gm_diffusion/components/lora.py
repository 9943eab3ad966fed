"""
LoRA adapters for the UNet: reading the checkpoint conventions in the wild into ONE canonical form.  Host-only (torch on the CPU,
no HIP): the device side is ``UNet2DConditionModel.load_lora`` and ``hip_ops.lora_update``.

diffusers and peft are not dependencies of this package, so the three key conventions below are this repository's restatement of
what their loaders accept (diffusers ``LoraLoaderMixin.lora_state_dict`` and its kohya conversion), not an import:

  PEFT / current diffusers   [unet.]<module>.lora_A.weight  [r, in]     [unet.]<module>.lora_B.weight  [out, r]    [<module>.alpha]
  older diffusers            [unet.]<module>.lora.down.weight           [unet.]<module>.lora.up.weight
                             [unet.]<block>.attn1.processor.to_q_lora.down.weight / .up.weight   (to_out_lora -> to_out.0)
  kohya                      lora_unet_<module with "." -> "_">.lora_down.weight / .lora_up.weight / .alpha

A module's update is  W + scale * (alpha / r) * up @ down  (factor 1 without an alpha).  kohya names are resolved against the model's
OWN module names with the dots replaced -- never by splitting on underscores, which ``to_out_0`` and ``transformer_blocks_0`` defeat.

What the UNet applies by default (``targets="attention"``, ``SUPPORTED_SUFFIXES``): the eight attention projections of every
BasicTransformerBlock -- the target set of diffusers' train_text_to_image_lora.py.  ``targets="transformer"`` (opt-in) adds the
other linears of a Transformer2DModel (``TRANSFORMER_SUFFIXES``): the feed-forward's ``ff.net.0.proj`` and ``ff.net.2`` and the
transformer's ``proj_in`` / ``proj_out`` -- what kohya's default settings and PEFT's wider ``target_modules`` train; the 4-D factors
kohya / LoCon write for a 1x1-convolution proj_in / proj_out are squeezed to matrices.  Everything else is refused BY NAME
(``NotImplementedError``) unless ``ignore_unsupported``, which skips it with one warning listing the modules: a silently thinner
adapter is never the default.
"""
import re
import warnings

import torch

from ..hip_ops import LORA_MAX_RANK as MAX_RANK  # the kernel's limit; importing hip_ops needs no GPU

SUPPORTED_SUFFIXES = tuple(f"{a}.{p}" for a in ("attn1", "attn2") for p in ("to_q", "to_k", "to_v", "to_out.0"))
FF_SUFFIXES = ("ff.net.0.proj", "ff.net.2")
PROJ_SUFFIXES = ("proj_in", "proj_out")
TRANSFORMER_SUFFIXES = SUPPORTED_SUFFIXES + FF_SUFFIXES + PROJ_SUFFIXES
TARGETS = ("attention", "transformer")

# key fragments of adapter families that are no plain linear LoRA at all
_FOREIGN = ("hada_", "lokr_", "dora_scale", "lora_mid", "lora_magnitude_vector")
_TEXT_PREFIXES = ("text_encoder.", "text_encoder_2.", "lora_te_", "lora_te1_", "lora_te2_")

_DOWN, _UP, _ALPHA = "down", "up", "alpha"
# (suffix of the key, which part it is); longest first
_PARTS = ((".lora_A.weight", _DOWN), (".lora_B.weight", _UP), (".lora.down.weight", _DOWN), (".lora.up.weight", _UP),
          (".lora_down.weight", _DOWN), (".lora_up.weight", _UP), (".alpha", _ALPHA))
_PROCESSOR = re.compile(r"^(.*)\.processor\.(to_q|to_k|to_v|to_out)_lora\.(down|up)\.weight$")


class LoraAdapterError(ValueError, NotImplementedError):
    """A call names an adapter that cannot be addressed: a name or an adapter that is already loaded, a name that is not loaded, a
    state dict without factors.  A ``ValueError`` -- the arguments are wrong -- that is ALSO a ``NotImplementedError``: while one
    adapter at a time was implemented, ``set_adapters``, ``adapter_name=`` and a second ``load_lora`` raised that, and callers that
    catch it keep working (the idiom of ``io.UnsupportedOperation``, an ``OSError`` and a ``ValueError``)."""


def same_adapter(p, q):
    """Do two parsed adapters ({module: (A, B, alpha)}) hold the same factors on the same modules?"""
    return p.keys() == q.keys() and all(p[m][2] == q[m][2] and p[m][0].shape == q[m][0].shape and torch.equal(p[m][0], q[m][0])
                                        and torch.equal(p[m][1], q[m][1]) for m in p)


def _check_targets(targets):
    if targets not in TARGETS:
        raise ValueError(f"LoRA: targets={targets!r} is not one of {TARGETS}")
    return targets


def _is_transformer_proj(module):
    """proj_in / proj_out of a Transformer2DModel (``...attentions.N.proj_in``), not a module that merely ends alike."""
    head, _, leaf = module.rpartition(".")
    return leaf in PROJ_SUFFIXES and re.search(r"attentions\.\d+$", head) is not None


def supported(module, targets="attention"):
    """Is ``module`` one of the projections the UNet applies an adapter to under ``targets``?"""
    _check_targets(targets)
    if ".transformer_blocks." in module and module.endswith(SUPPORTED_SUFFIXES):
        return True
    if targets == "attention":
        return False
    return (".transformer_blocks." in module and module.endswith(FF_SUFFIXES)) or _is_transformer_proj(module)


_OPT_IN = " -- pass targets='transformer' to apply it"


def _why_unsupported(module):
    if ".ff.net." in module:
        return "feed-forward target (the GEGLU kernel is fused)" + _OPT_IN
    if module.endswith(("proj_in", "proj_out")):
        return "proj_in / proj_out target" + _OPT_IN
    if "resnets." in module or module.endswith(("time_emb_proj", "conv1", "conv2", "conv_shortcut", "conv", "conv_in", "conv_out")):
        return "resnet / convolution target"
    return "not an attention projection of a transformer block"


def _split_key(key):
    """key -> (module name as written, part) or None when the key is no LoRA tensor."""
    m = _PROCESSOR.match(key)
    if m:
        proj = "to_out.0" if m.group(2) == "to_out" else m.group(2)
        return f"{m.group(1)}.{proj}", m.group(3)
    for suf, part in _PARTS:
        if key.endswith(suf):
            return key[: -len(suf)], part
    return None


def parse_lora_state_dict(sd, module_names, ignore_unsupported=False, targets="attention"):
    """``sd``: a LoRA checkpoint in any of the three conventions (module docstring); ``module_names``: the model's own module names
    (``down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q``, ...).  Returns ``{module: (A [r, K], B [N, r], alpha or None)}``
    with float32 CPU factors, for the modules supported under ``targets`` ("attention": the eight attention projections;
    "transformer": also ff.net.0.proj, ff.net.2, proj_in and proj_out, whose 1x1-convolution factors [r, in, 1, 1] / [out, r, 1, 1] are
    squeezed).  Unsupported modules, foreign adapter families, text-encoder keys and ranks above 128 raise ``NotImplementedError``
    naming the module; with ``ignore_unsupported`` they are skipped and ONE warning lists them."""
    _check_targets(targets)
    module_names = list(module_names)
    by_flat = {}
    for n in module_names:
        by_flat.setdefault(n.replace(".", "_"), n)
    known = set(module_names)
    parts, refused = {}, {}

    def refuse(name, why):
        refused.setdefault(name, why)

    for key, val in sd.items():
        if key.startswith(_TEXT_PREFIXES):
            refuse(key.split(".lora")[0], "text-encoder LoRA (the text tower is not adapted)")
            continue
        if any(f in key for f in _FOREIGN):
            refuse(key.rsplit(".", 1)[0] if "." in key else key, "LoHa / LoKr / DoRA / conv-LoRA key (only plain linear LoRA factors are applied)")
            continue
        sp = _split_key(key)
        if sp is None:
            refuse(key, "not a LoRA tensor (no lora_A / lora_B / lora.down / lora.up / lora_down / lora_up / alpha suffix; stray metadata "
                        "counts as an unsupported entry, so that nothing of a checkpoint is dropped silently)")
            continue
        name, part = sp
        if name.startswith("lora_unet_"):  # kohya: through the module table
            flat = name[len("lora_unet_"):]
            if flat not in by_flat:
                refuse(name, "no module of this UNet has that flattened name")
                continue
            name = by_flat[flat]
        else:
            if name.startswith("unet."):
                name = name[len("unet."):]
            if name not in known:
                refuse(name, "no module of this UNet has that name")
                continue
        parts.setdefault(name, {})[part] = val

    out = {}
    for name, p in parts.items():
        if not supported(name, targets):
            refuse(name, _why_unsupported(name))
            continue
        if _DOWN not in p or _UP not in p:
            raise KeyError(f"LoRA: module {name} has {sorted(p)} -- both the down (lora_A) and the up (lora_B) factor are needed")
        a, b = p[_DOWN], p[_UP]
        if _is_transformer_proj(name) and a.dim() == 4 and b.dim() == 4 and tuple(a.shape[2:]) == tuple(b.shape[2:]) == (1, 1):
            a, b = a[:, :, 0, 0], b[:, :, 0, 0]  # kohya / LoCon factors of a 1x1 convolution: the same matrices on tokens
        if a.dim() != 2 or b.dim() != 2:
            refuse(name, f"factors of shape {tuple(a.shape)} / {tuple(b.shape)}: convolution LoRA")
            continue
        if b.shape[1] != a.shape[0]:
            raise ValueError(f"LoRA: module {name}: down {tuple(a.shape)} and up {tuple(b.shape)} disagree on the rank")
        r = a.shape[0]
        if not 1 <= r <= MAX_RANK:
            refuse(name, f"rank {r} outside [1, {MAX_RANK}]")
            continue
        alpha = p.get(_ALPHA)
        alpha = None if alpha is None else float(alpha)
        out[name] = (a.detach().to("cpu", torch.float32).contiguous(), b.detach().to("cpu", torch.float32).contiguous(), alpha)

    if refused:
        listing = "; ".join(f"{n}: {w}" for n, w in sorted(refused.items()))
        if not ignore_unsupported:
            raise NotImplementedError(f"LoRA: {len(refused)} target(s) are not implemented -- {listing}.  Pass ignore_unsupported=True to "
                                      "apply the adapter without them.")
        warnings.warn(f"LoRA: skipped {len(refused)} unsupported target(s) -- {listing}", stacklevel=2)
    return out


def factor(rank, alpha):
    """The adapter's own factor alpha / r (1 without an alpha)."""
    return 1.0 if alpha is None else float(alpha) / rank


# ---------------------------------------------------------------------------------------------------------------------------
# several adapters at once: the host-side packing (pure CPU: tests/test_lora_multi_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
class ModulePacking:
    """One adapted module: ``adapters`` (load order), their ``ranks``, the column ``ranges`` [c0, c1) of each in the tightly packed
    stack, ``rank`` (the sum), ``padded`` (the sum rounded up to the multiple), ``slots`` (each adapter's entry in the table of scalar
    scales) and ``row`` (the module's row in the table of column scales; None for a module with ONE adapter, which keeps the
    single-adapter launch)."""

    def __init__(self, adapters, ranks, ranges, padded, slots, row):
        self.adapters, self.ranks, self.ranges, self.padded, self.slots, self.row = adapters, ranks, ranges, padded, slots, row
        self.rank = sum(ranks)

    @property
    def stacked(self):
        return self.row is not None


class Packing:
    """``modules``: {module: ModulePacking} in sorted module order; ``slots``: [(module, adapter)] -- one scalar scale each, sorted by
    module, then load order (ONE adapter: slot i is module i, today's table); ``rows`` / ``width``: the table of column scales holds
    one row per stacked module, ``width`` = the largest padded stacked rank."""

    def __init__(self, modules, slots, rows, width):
        self.modules, self.slots, self.rows, self.width = modules, slots, rows, width


def pack_adapters(adapters, multiple=32, limit=None):
    """``adapters``: {adapter name: {module: (A [r, K], B [N, r], alpha or None)}} in LOAD order (``parse_lora_state_dict`` each).
    Returns the ``Packing``: a module targeted by one adapter keeps its single launch; a module targeted by two or more gets their
    factors packed tightly along the rank, in load order, and the padding (to ``multiple``) applies to the SUM.  A padded sum above
    ``limit`` (default: the stacked kernel's 256) raises ``NotImplementedError`` naming the module, the ranks and the limit."""
    from ..hip_ops import LORA_MAX_STACKED_RANK

    limit = LORA_MAX_STACKED_RANK if limit is None else limit
    names = sorted({m for parsed in adapters.values() for m in parsed})
    modules, slots, rows, width = {}, [], 0, 0
    for m in names:
        who = [n for n, parsed in adapters.items() if m in parsed]
        ranks = [adapters[n][m][0].shape[0] for n in who]
        padded = -(-sum(ranks) // multiple) * multiple
        if len(who) > 1 and padded > limit:
            raise NotImplementedError(f"LoRA: module {m}: the ranks {' + '.join(str(r) for r in ranks)} of adapters {who} sum to {sum(ranks)} "
                                      f"(padded {padded}), above the stacked kernel's limit of {limit}")
        ranges, c = [], 0
        for r in ranks:
            ranges.append((c, c + r))
            c += r
        row = None
        if len(who) > 1:
            row, rows, width = rows, rows + 1, max(width, padded)
        modules[m] = ModulePacking(who, ranks, ranges, padded, list(range(len(slots), len(slots) + len(who))), row)
        slots.extend((m, n) for n in who)
    return Packing(modules, slots, rows, width)


def stack_factors(adapters, module, mp):
    """The stacked factors of ``module`` (``mp``: its ModulePacking): (A [padded, K], B [N, padded]) float32, adapter a at columns
    ``mp.ranges[a]``, zeros beyond the sum."""
    a0, b0, _ = adapters[mp.adapters[0]][module]
    a, b = torch.zeros(mp.padded, a0.shape[1]), torch.zeros(b0.shape[0], mp.padded)
    for n, (c0, c1) in zip(mp.adapters, mp.ranges):
        a[c0:c1], b[:, c0:c1] = adapters[n][module][0], adapters[n][module][1]
    return a, b


def scale_tables(adapters, packing, weights, scale=1.0):
    """The two float32 tables the kernels read: ``scalars`` [len(slots)], entry (module, a) = scale * weights[a] * alpha_a / r_a, and
    ``columns`` [rows, width] (at least [1, 1]), the row of a stacked module holding that very number on adapter a's columns and 0 on
    the pad columns.  An adapter missing from ``weights`` has weight 0.  Each entry is float32(alpha / r) * float32(scale * weight),
    one float32 product: with weight 1 the very number the single-adapter table has always held."""
    def f32(values):
        return torch.tensor(values, dtype=torch.float32)

    def sw(n):
        return float(scale) * float(weights.get(n, 0.0))

    def fac(m, n):
        a, _, alpha = adapters[n][m]
        return factor(a.shape[0], alpha)

    scalars = f32([fac(m, n) for m, n in packing.slots]) * f32([sw(n) for _, n in packing.slots])
    columns = torch.zeros(max(packing.rows, 1), max(packing.width, 1), dtype=torch.float32)
    for m, mp in packing.modules.items():
        if mp.stacked:
            for n, (c0, c1) in zip(mp.adapters, mp.ranges):
                columns[mp.row, c0:c1] = f32([fac(m, n)]) * f32([sw(n)])
    return scalars, columns


def load_lora_file(path_or_state_dict, weight_name=None, subfolder=None):
    """A LoRA checkpoint from a dict, a file or a directory (+ ``subfolder`` / ``weight_name``): local ``.safetensors``, or ``.bin`` /
    ``.pt`` with ``weights_only=True``.  Nothing is ever downloaded."""
    import os

    if isinstance(path_or_state_dict, dict):
        return path_or_state_dict
    path = os.fspath(path_or_state_dict)
    if subfolder:
        path = os.path.join(path, subfolder)
    if os.path.isdir(path):
        names = [weight_name] if weight_name else ["pytorch_lora_weights.safetensors", "pytorch_lora_weights.bin"]
        for n in names:
            if os.path.isfile(os.path.join(path, n)):
                path = os.path.join(path, n)
                break
        else:
            raise FileNotFoundError(f"load_lora_weights: none of {names} in {path} (local files only: nothing is downloaded)")
    elif weight_name and not os.path.isfile(path):
        path = os.path.join(path, weight_name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"load_lora_weights: {path} does not exist (local files only: nothing is downloaded)")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)
