"""LoRA adapters for ``MoDeDiT``: rank-r updates ``W + s B A`` of the four large matrices of every block on a frozen base.

In bf16 compute every launch chain (training forward, the backward's data-gradient GEMMs, every sampler and rollout graph) reads the bf16
shadow ``ParamArena.lp`` only, and the backward chain writes the dense weight gradient of every matrix into a flat fp32 buffer with the arena's
layout.  So an adapter needs no kernel of the chains changed:

* ``mode_lora_merge`` writes ``bf16(W + s B A)`` from the frozen fp32 master into the shadow - same pointers, so captured graphs keep replaying;
* ``mode_lora_grad`` projects the chain's ``dW`` onto the adapter, ``dA = s B^T dW`` and ``dB = s dW A^T`` (the chain rule of ``W + s B A``).

That is ``grad="dense"``: the chain still computes and writes the dense ``dW`` of all four matrices of every block into an arena-sized scratch.
``grad="factored"`` runs ``mode_dit_backward_lora`` instead: the chain rule factors through the low rank - with ``Y = X W_eff^T``,
``dA = s (dY B)^T X`` and ``dB = s dY^T (X A^T)`` - so the four weight-gradient GEMMs of every block are not launched at all, an adapted kind gets one
``mode_lora_fact_grad`` over the very bf16 operands its GEMM would have read, no ``rows x cols`` tensor is written and the arena-sized scratch is not
allocated (the chain's remaining small gradients go to a buffer of their own size).
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, List, Tuple

import torch
from torch import nn

from . import _lib as L
from .engine import _stream

TARGETS = ("wqkv", "wo", "w1", "w2")
GRAD_MODES = ("dense", "factored")


def target_shapes(model) -> Dict[str, Tuple[int, int, int]]:
    """Arena key of a block's matrix -> (G, rows, cols): the layout of ``arena._layer_keys``."""
    D, E = model.embed_dim, model.num_experts
    return {"wqkv": (1, 3 * D, D), "wo": (1, D, D), "w1": (E, 8 * D, D), "w2": (E, D, 4 * D)}


class LoraAdapter(nn.Module):
    """``LoraAdapter(model, rank=16, alpha=None, targets=("wqkv", "wo", "w1", "w2"), seed=0, grad="dense")``: per target kind ``A_<kind> [L, G, r, cols]`` ~
    N(0, 1/r) from ``seed`` and ``B_<kind> [L, G, rows, r]`` = 0, ordinary parameters of THIS module (G = experts for ``w1`` / ``w2``, else 1);
    ``s = alpha / rank``, ``alpha`` defaults to ``rank``.  The adapter is not a submodule of the model: ``model.named_parameters()`` and
    ``model.state_dict()`` keep the reference's layout.

    ``attach()`` freezes every parameter of the model (remembering the flags), registers the adapter as ``model._lora`` - replacing an adapter
    attached before, one at a time - and makes the bf16 shadow the merged weights.  From then on the engine re-merges wherever it would have
    re-cast the shadow: the adapter's parameter versions are part of ``DitEngine._key()``, so an optimizer step on the adapter, a
    ``load_state_dict`` or a change of ``alpha`` is picked up by the next forward, the training chain and graphed samplers alike, without a
    recapture.  Training: ``loss.backward()`` returns ``dA`` / ``dB`` through autograd (``training.py``); the base parameters' ``.grad`` stay None.
    ``detach()`` restores flags and the plain cast; ``fold()`` adds ``s B A`` into the fp32 master in place and detaches, after which the model
    saves in the reference's ``state_dict`` layout.  ``forward`` is the model's, so a wrapper that drives a module (torch DDP over the adapter
    alone) exchanges the adapter's gradients only.

    ``grad`` says how ``dA`` / ``dB`` are computed, not what the adapter is: ``"dense"`` projects the chain's dense weight gradients
    (``mode_lora_grad``, an arena-sized scratch per model), ``"factored"`` computes them from the GEMM operands inside the backward chain
    (``mode_dit_backward_lora``: no dense weight gradient, no such scratch).  A plain attribute, validated, that may change between steps; it is
    not part of ``state_dict()`` or of the merge key, and a file saved in one mode loads in the other.

    Refused with an error before anything changes: ``compute_dtype="fp32"`` (its GEMMs read the master), a ``FusedAdamW`` of the model (either
    order) and an ``ArenaEMA`` of the base.  Adapters on routers, embeddings or encoders, several adapters at once and the ZeRO-1 /
    ``fuse_expert_step`` combinations are out of scope."""

    def __init__(self, model, rank: int = 16, alpha=None, targets=TARGETS, seed: int = 0, grad: str = "dense"):
        super().__init__()
        self.grad = grad
        rank = int(rank)
        if not 1 <= rank <= L.MODE_LORA_MAX_RANK:
            raise ValueError(f"LoraAdapter: rank must be in 1..{L.MODE_LORA_MAX_RANK}, got {rank}")
        targets = tuple(targets)
        shapes = target_shapes(model)
        bad = [t for t in targets if t not in shapes]
        if bad or not targets or len(set(targets)) != len(targets):
            raise ValueError(f"LoraAdapter: targets must be distinct names out of {TARGETS}, got {targets}")
        if model.embed_dim % 8:
            raise ValueError("LoraAdapter: embed_dim must be a multiple of 8 (16-byte accesses of the merge and projection kernels)")
        self.__dict__["model"] = model                           # a plain reference: the model must not become a submodule of its adapter
        self.rank, self.targets = rank, tuple(t for t in TARGETS if t in targets)
        self.dims = dict(embed_dim=model.embed_dim, num_layers=model.num_layers, num_experts=model.num_experts)
        dev = next(model.parameters()).device
        gen = torch.Generator().manual_seed(int(seed))
        Ly = model.num_layers
        for t in self.targets:
            G, rows, cols = shapes[t]
            a = torch.randn(Ly, G, rank, cols, generator=gen) * rank ** -0.5
            setattr(self, f"A_{t}", nn.Parameter(a.to(dev)))
            setattr(self, f"B_{t}", nn.Parameter(torch.zeros(Ly, G, rows, rank, device=dev)))
        self._alpha = float(rank if alpha is None else alpha)
        self._scale = None                                       # device fp32 scalar, made on first use (the kernels read s from memory)
        self._gen = 0                                            # bumped by what changes the merge without touching a parameter (alpha)
        self._attached = False
        self._saved_flags: List[Tuple[nn.Parameter, bool]] = []

    # ------------------------------------------------------------------ gradient mode
    @property
    def grad(self) -> str:
        return self._grad

    @grad.setter
    def grad(self, value) -> None:
        if value not in GRAD_MODES:
            raise ValueError(f"LoraAdapter: grad must be one of {GRAD_MODES}, got {value!r}")
        self._grad = value

    # ------------------------------------------------------------------ scale
    @property
    def alpha(self) -> float:
        return self._alpha

    @alpha.setter
    def alpha(self, value) -> None:
        self._alpha = float(value)
        if self._scale is not None:
            self._scale.fill_(self._alpha / self.rank)
        self._gen += 1

    @property
    def scale(self) -> float:
        return self._alpha / self.rank

    def _scale_dev(self, dev) -> torch.Tensor:
        if self._scale is None or self._scale.device != dev:
            self._scale = torch.full((1,), self._alpha / self.rank, dtype=torch.float32, device=dev)
        return self._scale

    def pairs(self):
        """[(target, A, B)] in the fixed target order."""
        return [(t, getattr(self, f"A_{t}"), getattr(self, f"B_{t}")) for t in self.targets]

    def forward(self, *args, **kwargs):
        return self.model(*args, **kwargs)

    # ------------------------------------------------------------------ attach / detach
    def _refuse(self) -> None:
        m = self.model
        if m.compute_dtype != "bf16":
            raise ValueError("LoraAdapter needs compute_dtype='bf16': the fp32 GEMMs read the master weights, and a second fp32 copy of the model "
                             "is out of scope")
        ref = _FUSED_ADAMW.get(m)
        if ref is not None and ref() is not None:
            raise RuntimeError("LoraAdapter.attach(): this model has a FusedAdamW, which steps the frozen base and writes the shadow itself - drop "
                               "it and train the adapter with FlatAdamW(adapter.parameters(), ...)")
        for t, a, b in self.pairs():
            if a.dtype != torch.float32 or b.dtype != torch.float32 or not a.is_contiguous() or not b.is_contiguous():
                raise ValueError(f"LoraAdapter: A_{t} / B_{t} must be dense fp32 tensors")

    def attach(self) -> "LoraAdapter":
        m = self.model
        self._refuse()
        prev = m.__dict__.get("_lora")
        if prev is self:
            return self
        if prev is not None:
            # hot swap: the flags saved by the first adapter pass on and only the shadow changes - _merge_into re-casts what the previous
            # adapter targeted and this one does not, then merges this one's targets
            self._saved_flags, prev._saved_flags = prev._saved_flags, []
            prev._attached = False
        else:
            self._saved_flags = [(p, p.requires_grad) for p in m.parameters()]
            for p, _ in self._saved_flags:
                p.requires_grad = False
        m.__dict__["_lora"] = self                               # (not through Module.__setattr__: that would register a submodule)
        self._attached = True
        if next(m.parameters()).is_cuda:
            m.engine                                             # noqa: B018 - ensure_weights() merges now
        return self

    def detach(self) -> None:
        m = self.model
        if m.__dict__.get("_lora") is not self:
            return
        del m.__dict__["_lora"]
        self._attached = False
        for p, flag in self._saved_flags:
            p.requires_grad = flag
        self._saved_flags = []
        eng = m._engine
        if eng is not None:
            eng._lora_bufs.clear()                               # the model's projection scratch (arena-sized) goes with its last adapter
            if eng.arena is not None:
                eng.arena.lp_synced = False                      # the next ensure_weights() re-casts the whole arena
                eng.arena.lora_merged = ()
                eng.arena.version += 1

    def merge(self) -> None:
        """Re-merge now (the engine does so by itself whenever the adapter's parameters, ``alpha`` or the base changed)."""
        if not self._attached:
            raise RuntimeError("LoraAdapter.merge(): not attached")
        self._gen += 1                                           # the key changes: the engine access below merges exactly once
        self.model.engine                                        # noqa: B018

    @torch.no_grad()
    def fold(self) -> None:
        """``W += s B A`` in the fp32 master, in place, then ``detach()``: the model is a plain fine-tuned ``MoDeDiT`` again."""
        if not self._attached:
            raise RuntimeError("LoraAdapter.fold(): not attached")
        eng = self.model.engine
        self._launch_merge(eng, into_master=True)
        self.detach()
        eng.weights_updated(lp_synced=False)

    # ------------------------------------------------------------------ engine side
    def _key(self):
        ps = self.__dict__.get("_plist")                         # the parameter objects are fixed at construction: no module walk per engine access
        if ps is None:
            ps = self.__dict__["_plist"] = list(self.parameters())
        return (id(self), self._gen, tuple(p._version for p in ps), tuple(p.data_ptr() for p in ps))

    def _descs(self, eng):
        """(target, layer, ModeLoraDesc with the shapes, strides and adapter pointers filled in, arena key)."""
        m, dev = self.model, eng.device
        shapes = target_shapes(m)
        s = self._scale_dev(dev)
        out = []
        for t, a, b in self.pairs():
            if a.device != dev or b.device != dev:
                raise RuntimeError(f"LoraAdapter: A_{t} / B_{t} live on {a.device}, the model on {dev} - move the adapter with .to()")
            G, rows, cols = shapes[t]
            for i in range(m.num_layers):
                d = L.ModeLoraDesc(G=G, rows=rows, cols=cols, r=self.rank, w_stride=rows * cols, A=a[i].data_ptr(), B=b[i].data_ptr(), scale=s.data_ptr())
                out.append((t, i, d, f"l{i}.{t}"))
        return out

    def _launch_merge(self, eng, into_master: bool) -> None:
        ar = eng.arena
        for t, i, d, key in self._descs(eng):
            d.W = ar.w[key].data_ptr()
            d.out = ar.w[key].data_ptr() if into_master else ar.wl[key].data_ptr()
            d.out_dtype = L.MODE_F32 if into_master else L.MODE_BF16
            L.check(eng.lib.mode_lora_merge(C.byref(d), _stream()), f"lora_merge {key}")

    def _merge_into(self, eng) -> None:
        """Called by ``DitEngine.ensure_weights`` after the cast: the targeted slices of the shadow become bf16(W + s B A)."""
        if eng.compute_dtype != "bf16":
            raise ValueError("a LoraAdapter is attached: compute_dtype must stay 'bf16'")
        ar = eng.arena
        # what an adapter attached before merged into tensors this one does not target goes back to the plain cast (a whole-arena cast by
        # ensure_lp just now did that already; casting those slices again changes nothing)
        for t in getattr(ar, "lora_merged", ()):
            if t not in self.targets:
                for i in range(self.model.num_layers):
                    ar.wl[f"l{i}.{t}"].copy_(ar.w[f"l{i}.{t}"])
        self._launch_merge(eng, into_master=False)
        ar.lora_merged = self.targets

    @staticmethod
    def grad_scratch(eng) -> torch.Tensor:
        """The flat buffer the backward chain writes its dense gradients into while an adapter is attached.  One per MODEL (held by its engine, shared
        by every adapter of the model, released when the last one detaches): it is as large as the arena, an adapter is not."""
        n, dev = eng.arena.bounds["total"], eng.device
        eng._lora_bufs.pop("small", None); eng._lora_bufs.pop("fact_ws", None)         # left by grad="factored"
        flat = eng._lora_bufs.get("flat")
        if flat is None or flat.numel() != n or flat.device != dev:
            flat = eng._lora_bufs["flat"] = torch.empty(n, dtype=torch.float32, device=dev)
        return flat

    def project(self, eng, flat: torch.Tensor, params) -> list:
        """``mode_lora_grad`` over every layer and target of ``flat`` (arena layout); returns the gradients of ``params`` (a subset of this
        adapter's parameters, by identity; None for one that is not an adapter tensor)."""
        ar = eng.arena
        views = ar._views(flat)
        grads = {}
        for t, a, b in self.pairs():
            grads[id(a)], grads[id(b)] = torch.empty_like(a), torch.empty_like(b)
        descs = self._descs(eng)
        need = max(eng.lib.mode_lora_grad_workspace_bytes(C.byref(d)) for _, _, d, _ in descs)
        ws = eng._lora_bufs.get("ws")                            # the partials' workspace: per model as well
        if ws is None or ws.numel() < need or ws.device != eng.device:
            ws = eng._lora_bufs["ws"] = torch.empty(need, dtype=torch.uint8, device=eng.device)
        for t, i, d, key in descs:
            d.dW = views[key].data_ptr()
            d.dA = grads[id(getattr(self, f"A_{t}"))][i].data_ptr()
            d.dB = grads[id(getattr(self, f"B_{t}"))][i].data_ptr()
            L.check(eng.lib.mode_lora_grad(C.byref(d), ws.data_ptr(), ws.numel(), _stream()), f"lora_grad {key}")
        return [grads.get(id(p)) for p in params]

    # ------------------------------------------------------------------ grad="factored"
    @staticmethod
    def small_grad_scratch(eng) -> torch.Tensor:
        """The buffer of the chain's remaining gradients (biases, gains, routers, embeddings, head) in factored mode: ``small_grad_layout``, a few
        MB.  Per model like the dense scratch, which is dropped here - a model that switches to factored mode gives its 2.7 GB back."""
        eng._lora_bufs.pop("flat", None); eng._lora_bufs.pop("ws", None)
        n, dev = small_grad_layout(eng.arena)[1], eng.device
        buf = eng._lora_bufs.get("small")
        if buf is None or buf.numel() != n or buf.device != dev:
            buf = eng._lora_bufs["small"] = torch.empty(n, dtype=torch.float32, device=dev)
        return buf

    def fact_tables(self, eng, B: int, params):
        """(ModeLoraTrain for one backward at batch size B, the gradients of ``params`` it will write, what must stay alive over the call).  The A / B
        pointer tables are built once per set of adapter tensors (keyed by their ``data_ptr()``), the dA / dB tables per backward: the gradients are
        fresh ``empty_like`` tensors handed to autograd, as ``project()``'s are."""
        m, dev = self.model, eng.device
        Ly = m.num_layers
        key = tuple(p.data_ptr() for _, a, b in self.pairs() for p in (a, b))
        hit = self.__dict__.get("_fact_cache")
        if hit is None or hit[0] != key:
            tabs = {}
            for t, a, b in self.pairs():
                if a.device != dev or b.device != dev:
                    raise RuntimeError(f"LoraAdapter: A_{t} / B_{t} live on {a.device}, the model on {dev} - move the adapter with .to()")
                tabs[t] = ((C.c_void_p * Ly)(*[a[i].data_ptr() for i in range(Ly)]), (C.c_void_p * Ly)(*[b[i].data_ptr() for i in range(Ly)]))
            hit = self.__dict__["_fact_cache"] = (key, tabs)
        tabs = hit[1]
        need = eng.lib.mode_dit_backward_lora_workspace_bytes(C.byref(eng.dims), B, self.rank)
        if need == 0:
            raise ValueError("LoraAdapter(grad='factored'): the backward chain refuses this model geometry (embed_dim must be a multiple of 8)")
        ws = eng._lora_bufs.get("fact_ws")
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = eng._lora_bufs["fact_ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        lt = L.ModeLoraTrain(r=self.rank, scale=self._scale_dev(dev).data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel())
        grads, keep = {}, [tabs]
        for t, a, b in self.pairs():
            ga, gb = torch.empty_like(a), torch.empty_like(b)
            grads[id(a)], grads[id(b)] = ga, gb
            da = (C.c_void_p * Ly)(*[ga[i].data_ptr() for i in range(Ly)])
            db = (C.c_void_p * Ly)(*[gb[i].data_ptr() for i in range(Ly)])
            keep += [da, db]
            kd = L.LORA_KINDS.index(t)
            lt.A[kd], lt.B[kd] = C.cast(tabs[t][0], C.c_void_p), C.cast(tabs[t][1], C.c_void_p)
            lt.dA[kd], lt.dB[kd] = C.cast(da, C.c_void_p), C.cast(db, C.c_void_p)
        return lt, [grads.get(id(p)) for p in params], (keep, list(grads.values()))

    # ------------------------------------------------------------------ serialisation
    def get_extra_state(self):
        return dict(rank=self.rank, alpha=self._alpha, targets=list(self.targets), **self.dims)

    def set_extra_state(self, state) -> None:
        self.alpha = float(state["alpha"])

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        meta = state_dict.get("_extra_state")
        if meta is None:
            raise ValueError("LoraAdapter.load_state_dict: no adapter description ('_extra_state') in this dict - not a LoraAdapter.state_dict()")
        mine = self.get_extra_state()
        diff = {k: (meta.get(k), mine[k]) for k in mine if k != "alpha" and meta.get(k) != mine[k]}
        if diff:
            raise ValueError("LoraAdapter.load_state_dict: the file was made for another adapter or model (file, this adapter): "
                             + ", ".join(f"{k}: {a} != {b}" for k, (a, b) in diff.items()))
        for k, v in self.state_dict().items():
            if k != "_extra_state" and (k not in state_dict or tuple(state_dict[k].shape) != tuple(v.shape)):
                raise ValueError(f"LoraAdapter.load_state_dict: tensor {k} is missing or has another shape than {tuple(v.shape)}")
        return super().load_state_dict(state_dict, strict=strict, **kw)


# model -> weak reference to its FusedAdamW: a registry beside the models, so that a model carries nothing for a feature it does not use (a copy
# of a model is not in it, and the model pickles as before)
_FUSED_ADAMW = weakref.WeakKeyDictionary()


def small_grad_layout(ar):
    """([(key, shape, offset)], total): the arena's gradient layout without the four matrices of every block (and the dead gripper embedding) -
    what the backward chain still writes when ``mode_dit_backward_lora`` skips the weight-gradient GEMMs.  Offsets in elements, 256-byte aligned."""
    out, off = [], 0
    for key, shp, _ in ar.layout:
        if key == "gripper" or (key.startswith("l") and key.split(".")[-1] in TARGETS):
            continue
        out.append((key, shp, off))
        off += (int(torch.Size(shp).numel()) + 63) // 64 * 64
    return out, off


def adapter_of(model):
    """The adapter attached to ``model`` or None."""
    return model.__dict__.get("_lora")


def note_fused_adamw(model, opt) -> None:
    """``FusedAdamW.__init__``: refuse a model with an adapter, and note the optimizer for ``attach()``."""
    if adapter_of(model) is not None:
        raise RuntimeError("FusedAdamW on a model with a LoraAdapter attached: the base is frozen - use FlatAdamW(adapter.parameters(), ...)")
    _FUSED_ADAMW[model] = weakref.ref(opt)
