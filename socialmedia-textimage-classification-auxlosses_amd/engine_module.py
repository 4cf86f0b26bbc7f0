"""Host-side machinery shared by the front ends over libmmhip.so (mm_late.py, mm_early.py, and one_tower.py under text_only.py and
image_only.py): parameters as views into flat fp32 buffers under the reference checkpoint's keys, the engine handle and its (re)creation when a
batch outgrows the capacity, the dropout seed counter, the guard words, and the trainer-side pieces every fused step shares.  Nothing here knows
an architecture: a front end names its C entry points (`_ABI`), builds its config struct, allocates its flat buffers, re-applies its per-handle
setters and binds (the hooks of EngineModule).
"""
import ctypes as C
import json
import math
import os

import torch
import torch.nn as nn

from . import _lib


def merge_ranges(spans):
    """(offset, numel) spans of a flat buffer -> their padded [offset, offset + ((numel + 3) & ~3)) ranges, merged where adjacent, in address
    order (every tensor of a layout starts 16-byte aligned, so neighbours meet at the padded end)"""
    out = []
    for b, e in sorted((o, o + ((n + 3) & ~3)) for o, n in spans):
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e)
        else:
            out.append((b, e))
    return out


def read_param_infos(count_fn, info_at_fn, handle):
    """the layout of a handle (include/mmhip.h mmhip_param_info) as a list of dicts, in layout order"""
    infos, pi = [], _lib.ParamInfo()
    for i in range(count_fn(handle)):
        _lib.check(info_at_fn(handle, i, C.byref(pi)), "param_info")
        infos.append(dict(name=pi.name.decode(), shape=tuple(pi.dims[: pi.ndim]), buffer=pi.buffer, group=pi.group, offset=int(pi.offset),
                          numel=int(pi.numel)))
    return infos


class _Node(nn.Module):
    """name-space node so that parameters carry the reference checkpoint's dotted keys"""


def register_flat_parameters(module, infos, flats):
    """nn.Parameters that are views into the flat fp32 buffers `flats[buffer]`, registered on `module` under the reference checkpoint's keys
    (inf["param"] is set); buffer 0 is the frozen one (the 'vision' parameters, reference mm_late.py:67-69)"""
    for inf in infos:
        view = flats[inf["buffer"]][inf["offset"]: inf["offset"] + inf["numel"]].view(inf["shape"])
        node, parts = module, inf["name"].split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, _Node())
            node = node._modules[part]
        inf["param"] = nn.Parameter(view, requires_grad=inf["buffer"] != 0)
        node.register_parameter(parts[-1], inf["param"])


def _read_hf_dir(path):
    """(config dict, state dict) of a local HuggingFace model directory, or (None, None)"""
    cfg_file = os.path.join(path, "config.json")
    if not os.path.isfile(cfg_file):
        return None, None
    with open(cfg_file) as f:
        cfg = json.load(f)
    sd = None
    if os.path.isfile(os.path.join(path, "model.safetensors")):
        from safetensors.torch import load_file
        sd = load_file(os.path.join(path, "model.safetensors"))
    elif os.path.isfile(os.path.join(path, "pytorch_model.bin")):
        sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu")
    return cfg, sd


class EngineModule(nn.Module):
    """nn.Module over one engine handle.  A subclass sets `device_`, calls `_init_engine(seed_base)` and then `_create_engine(*capacity)`, and
    provides the hooks below; it gets `_handle`, `_capacity`, `_ws`, `_infos`, `_stage_ranges` and the parameters."""

    # names of the family's entry points in include/mmhip.h: create, destroy, param_count, param_info_at, workspace_bytes, num_stages, stage_grad_range
    _ABI = {}

    def _config(self, *capacity):
        """the family's config struct for this capacity"""
        raise NotImplementedError

    def _allocate_flats(self, h):
        """first creation: allocate the flat parameter / gradient buffers; -> {param_info.buffer: flat parameter buffer}"""
        raise NotImplementedError

    def _on_registered(self):
        """first creation, parameters registered: whatever else lives as long as the module (device words the setters hand to each handle)"""

    def _apply_setters(self, h):
        """every creation: the per-handle setters -- a new handle knows nothing of what the old one was told"""

    def _before_workspace(self, h):
        """every creation: what changes the workspace size has to be said before it is asked for"""

    def _bind(self, h):
        """every creation: hand the flat buffers and self._ws to the handle"""
        raise NotImplementedError

    def _init_engine(self, seed_base):
        self._handle, self._ws, self._weights_version = None, None, None
        self._seed_base, self._calls, self._fwd_token, self._last, self._grad_dirty = seed_base, 0, 0, {}, False

    def _create_engine(self, *capacity):
        """a handle for `capacity`; the one before it (a batch outgrew it) is destroyed once the new one exists.  The flat buffers, the
        parameters and the device words outlive the handles; setters, workspace, binding and stage ranges are per handle."""
        lib, abi = _lib.lib(), self._ABI
        cfg, h = self._config(*capacity), C.c_void_p()
        _lib.check(getattr(lib, abi["create"])(C.byref(cfg), C.byref(h)), abi["create"][len("mmhip_"):])
        first = self._handle is None
        if not first:
            getattr(lib, abi["destroy"])(self._handle)
        self._handle = h
        self._capacity = tuple(int(c) for c in capacity)
        if first:
            flats = self._allocate_flats(h)
            self._infos = read_param_infos(getattr(lib, abi["param_count"]), getattr(lib, abi["param_info_at"]), h)
            register_flat_parameters(self, self._infos, flats)
            self._on_registered()
        self._apply_setters(h)
        self._ws = None
        torch.cuda.empty_cache()
        self._before_workspace(h)
        self._ws = torch.empty(getattr(lib, abi["workspace_bytes"])(h), dtype=torch.uint8, device=self.device_)
        if os.environ.get("MMHIP_POISON_WS"):       # debugging aid: no kernel may read workspace it has not written
            self._ws.fill_(int(os.environ["MMHIP_POISON_WS"], 0))
        self._bind(h)
        self._stage_ranges = []
        b, e = C.c_uint64(), C.c_uint64()
        for st in range(getattr(lib, abi["num_stages"])(h)):
            _lib.check(getattr(lib, abi["stage_grad_range"])(h, st, C.byref(b), C.byref(e)), "stage_grad_range")
            self._stage_ranges.append((int(b.value), int(e.value)))
        self._weights_version = None

    def __del__(self):
        try:
            if self._handle is not None:
                getattr(_lib.lib(), self._ABI["destroy"])(self._handle)
        except Exception:
            pass

    def _next_seed(self):
        """the dropout seed of the next engine call"""
        self._calls += 1
        return (self._seed_base * 0x9E3779B97F4A7C15 + self._calls) & 0xFFFFFFFFFFFFFFFF

    def _zero_grad_state(self):
        """the entry condition of include/mmhip.h's backward contract: zero gradient"""
        self._flat_grad.zero_()

    def _clean_grad(self):
        """an autograd-path backward left its gradient in the flat buffer (tests and callers inspect it): the fused step re-establishes its
        entry condition when it finds this mark"""
        if self._grad_dirty:
            self._zero_grad_state()
            self._grad_dirty = False


class GuardedEngineModule(EngineModule):
    """engines of the mmhip_handle kind (late fusion, text only, image only; include/mmhip.h: the per-handle setters take any of them): the guard
    words are device memory of the module that every handle is pointed at.  A subclass sets `backward_products` (None: the engine's default)."""

    _loss_scale = 0.0         # of the f16 gradients (0: the engine's own); the late-fusion trainer moves it
    _word_info = None         # no word table unless WordTableEngineModule finds one: FlatTrainer steps the whole buffer densely
    _grad_clip = None         # (max_norm, state block) while global-norm gradient clipping is armed (set_grad_clip)

    def _on_registered(self):
        # device words of every handle: [0:2] include/mmhip.h mmhip_set_guard {non-finite counter, void-step flag}; [2] the word table's
        self._guard4 = torch.zeros(4, dtype=torch.int32, device=self.device_)
        self._nonfinite = self._guard4[:2]

    def _apply_setters(self, h):
        lib = _lib.lib()
        _lib.check(lib.mmhip_set_guard(h, _lib.ptr(self._nonfinite)), "set_guard")
        if self.backward_products is not None:
            _lib.check(lib.mmhip_set_backward_products(h, self.backward_products), "set_backward_products")
        if self._grad_clip is not None:
            _lib.check(lib.mmhip_set_grad_clip(h, self._grad_clip[0], _lib.ptr(self._grad_clip[1])), "set_grad_clip")

    def set_grad_clip(self, max_norm):
        """arm global-norm gradient clipping of the fused steps at `max_norm` (include/mmhip.h mmhip_set_grad_clip), or disarm it with None.  The
        state block -- four public words {coef, norm, clipped steps, steps}, then the partial sums -- is device memory of the module, like the
        guard words: every handle is pointed at it."""
        lib = _lib.lib()
        if max_norm is None:
            self._grad_clip = None
            _lib.check(lib.mmhip_set_grad_clip(self._handle, 0.0, None), "set_grad_clip")
            return
        max_norm = float(max_norm)
        if not math.isfinite(max_norm) or max_norm <= 0.0:
            raise ValueError(f"max_grad_norm must be a positive finite number, got {max_norm!r}")
        state = self._grad_clip[1] if self._grad_clip is not None else torch.zeros(int(lib.mmhip_grad_clip_state_bytes()), dtype=torch.uint8, device=self.device_)
        _lib.check(lib.mmhip_set_grad_clip(self._handle, max_norm, _lib.ptr(state)), "set_grad_clip")
        self._grad_clip = (max_norm, state)


class WordTableEngineModule(GuardedEngineModule):
    """engines whose trainable buffer is closed by a word table stepped row-lazily (late fusion, text only): the row flags shared by the
    backward pass and mmhip_adamw_rows, like the guard words, are device memory of the module that every handle is pointed at"""

    _embeddings = ()          # module path of the text embeddings (they carry the position_ids buffer)

    def _on_registered(self):
        super()._on_registered()
        emb = self
        for part in self._embeddings:
            emb = emb._modules[part]
        # transformers 4.25.1 checkpoints carry this buffer
        emb.register_buffer("position_ids", torch.arange(self.arch["max_pos"], device=self.device_).unsqueeze(0))
        self._word_info = next(i for i in self._infos if i["name"].endswith("word_embeddings.weight"))
        self._word_row_state = torch.zeros((self._word_info["shape"][0] + 3) // 4 * 4, dtype=torch.uint8, device=self.device_)
        # mmhip_set_index_counter: token ids that had to be clamped into the word table (the reference raises IndexError for them)
        self._bad_index = self._guard4[2:3]

    def _apply_setters(self, h):
        super()._apply_setters(h)
        lib = _lib.lib()
        _lib.check(lib.mmhip_set_row_state(h, _lib.ptr(self._word_row_state)), "set_row_state")
        _lib.check(lib.mmhip_set_index_counter(h, _lib.ptr(self._bad_index)), "set_index_counter")
        if self._loss_scale > 0:
            _lib.check(lib.mmhip_set_loss_scale(h, self._loss_scale), "set_loss_scale")

    def _zero_grad_state(self):
        """... and no "row has a gradient" flags"""
        self._flat_grad.zero_()
        self._word_row_state.bitwise_and_(0xFE)


class FlatTrainer(object):
    """what the trainers over `self.model` (an EngineModule) share.  `_moments` / `_adamw_ranges` serve GuardedEngineModule models, with a word
    table (stepped row-lazily) or without one."""

    # ---- checkpoints: plain state_dict with the reference's keys
    def load_saved_model(self, model_path):
        self.model.load_state_dict(torch.load(model_path, map_location=self.device))

    def save_model(self, model_path):
        torch.save(self.model.state_dict(), model_path)

    @staticmethod
    def _class_weight(loss_fn, class_weight):
        """`loss_fn` is accepted for signature parity: the class weights ride on it (nn.CrossEntropyLoss(weight=w))"""
        if class_weight is None and loss_fn is not None and getattr(loss_fn, "weight", None) is not None:
            return loss_fn.weight
        return class_weight

    def _moments(self):
        m = self.model
        if self._opt is None:
            self._opt = (torch.zeros_like(m._flat_train), torch.zeros_like(m._flat_train))
            if m._word_info is not None:
                m._word_row_state.bitwise_and_(1)                  # fresh moments: no row has any yet
        return self._opt

    # ---- global-norm gradient clipping (opt-in: max_grad_norm=None builds nothing and calls nothing new)
    max_grad_norm = None      # the threshold while armed (set_max_grad_norm)

    @staticmethod
    def _refuse_grad_clip_under_dp(max_grad_norm, world_size):
        if max_grad_norm is not None and world_size > 1:
            raise NotImplementedError(
                f"max_grad_norm with a gradient exchange (world size {world_size}): the norm needs the whole summed gradient before the first AdamW launch, but under data "
                "parallelism the word-table rows arrive after the dense optimizer has run, and the sharded optimizer holds only its own shard -- it "
                "would need a sum of partial norms across ranks.  Data-parallel clipping is not implemented; run one process or drop the flag")

    def set_max_grad_norm(self, max_grad_norm):
        """arm global-norm gradient clipping of this trainer's steps at `max_grad_norm`, or disarm it with None (the constructors' keyword)"""
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if max_grad_norm is not None or getattr(self.model, "_grad_clip", None) is not None:
            self.model.set_grad_clip(self.max_grad_norm)

    def _grad_clip_norm(self, ranges, grad_scale):
        """staged form of the fused step's norm (include/mmhip.h mmhip_op_grad_clip): over the dense parts of `ranges` and the flagged word-table
        rows, before the first AdamW call of the step; nothing when clipping is not armed"""
        m = self.model
        if getattr(m, "_grad_clip", None) is None:
            return
        word = m._word_info
        w0 = word["offset"] if word is not None else float("inf")
        dense = [(b, min(e, w0)) for b, e in ranges if min(e, w0) > b]
        rows = word is not None and any(e > w0 for _, e in ranges)
        seg_g = (C.c_void_p * max(len(dense), 1))(*[m._flat_grad.data_ptr() + b * 4 for b, _ in dense])
        seg_n = (C.c_uint64 * max(len(dense), 1))(*[e - b for b, e in dense])
        V, H = word["shape"] if rows else (0, 4)
        _lib.check(_lib.lib().mmhip_op_grad_clip(seg_g, seg_n, len(dense), C.c_void_p(m._flat_grad.data_ptr() + w0 * 4) if rows else None, V, H,
                                                 _lib.ptr(m._word_row_state) if rows else None, m._grad_clip[0], grad_scale, _lib.ptr(m._nonfinite),
                                                 _lib.ptr(m._grad_clip[1]), _lib.stream_ptr()), "op_grad_clip")

    def grad_clip_stats(self):
        """{norm, coef, clipped_steps, steps} of the armed clip: the last step's norm (after grad_scale) and coefficient, and the counts since arming.
        Synchronises: for logs and tests.  None when clipping is not armed."""
        clip = getattr(self.model, "_grad_clip", None) if self.max_grad_norm is not None else None
        if clip is None:
            return None
        words = clip[1][:16].cpu()
        f, u = words.view(torch.float32), words.view(torch.int32)
        return dict(norm=float(f[1]), coef=float(f[0]), clipped_steps=int(u[2]), steps=int(u[3]))

    def _log_grad_clip(self):
        """train()'s line per epoch -- only when armed"""
        st = self.grad_clip_stats()
        if st is not None:
            print(f"grad clip (max_grad_norm {self.max_grad_norm:g}): last norm {st['norm']:.4g} coef {st['coef']:.4g}, "
                  f"clipped {st['clipped_steps']} of {st['steps']} steps")

    def _adamw_ranges(self, ranges, lr, weight_decay, step, grad_scale, dense=True, rows=True):
        """staged AdamW: the dense part of each range up to the word table, then the row-lazy word table (no word table: all of it is dense).
        With clipping armed (_grad_clip_norm has run) the calls carry the state block, as the fused step's launches do."""
        m, lib = self.model, _lib.lib()
        em, ev = self._moments()
        at = lambda t, el: C.c_void_p(t.data_ptr() + el * 4)
        word = m._word_info
        w0 = word["offset"] if word is not None else float("inf")    # the word table closes the trainable buffer
        adamw, adamw_rows, tail = lib.mmhip_adamw_guarded, lib.mmhip_adamw_rows_guarded, ()
        if getattr(m, "_grad_clip", None) is not None:
            adamw, adamw_rows, tail = lib.mmhip_adamw_clipped, lib.mmhip_adamw_rows_clipped, (_lib.ptr(m._grad_clip[1]),)
        for b, e in ranges:
            dense_end = min(e, w0)
            if dense and dense_end > b:
                _lib.check(adamw(at(m._flat_train, b), at(m._flat_grad, b), at(em, b), at(ev, b), dense_end - b, lr, 0.9, 0.999,
                                 1e-8, weight_decay, step, grad_scale, 1, _lib.stream_ptr(), _lib.ptr(m._nonfinite), *tail), "adamw")
            if rows and e > w0:
                # rows without gradient and without moments only decay: same values as the dense update, 1/4 of its traffic
                _lib.check(adamw_rows(at(m._flat_train, w0), at(m._flat_grad, w0), at(em, w0), at(ev, w0), *word["shape"],
                                      _lib.ptr(m._word_row_state), lr, 0.9, 0.999, 1e-8, weight_decay, step,
                                      grad_scale, 1, _lib.stream_ptr(), _lib.ptr(m._nonfinite), *tail), "adamw_rows")

    def _clamped_message(self, n):
        raise NotImplementedError

    def _raise_on_clamped_indices(self, count):
        """the engine clamps indices into their embedding tables and counts them (include/mmhip.h mmhip_set_index_counter): the reference's
        nn.Embedding raises IndexError for such an index, so does this for every count not yet reported"""
        seen = getattr(self, "_bad_seen", 0)
        if count > seen:
            self._bad_seen = count
            raise IndexError(self._clamped_message(count - seen))

    def check_indices(self):
        """synchronising form of the check (end of an epoch, an evaluation or a feature loop)"""
        self._raise_on_clamped_indices(int(self.model._bad_index.item()))
