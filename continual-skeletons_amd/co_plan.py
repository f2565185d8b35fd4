"""The native plan of a ``CoStGcn`` (csk_co_plan, include/cskel.h; csrc/executor.hip): one C call per cycle in the place of
the ~25 ctypes calls of the Python engine (continual.py).  What lives here: marshalling the ten blocks and the model-level
operands into ``csk_co_layer`` structs, the plan's lifetime, and the exact once-per-cycle check that the operands it holds
are still the model's weights.  The stepping position is NOT here: the plan steps on the model's counter buffer."""
import ctypes

import torch

from . import native
from .blocks import is_plain_graph_conv


class NativePlan:
    """Base class of ``CoStGcn``; its only state is the ``__dict__`` entries ``_plan`` (handle), ``_plan_keep`` (operands kept
    alive + weight slots), ``_weights_dirty`` / ``_dirty_hooks`` and the adaptive graph convs' ``_agcn_adj`` scratch."""

    def _mark_weights_dirty(self, *args, **kwargs):
        self.__dict__["_weights_dirty"] = True

    def _install_dirty_hooks(self):
        """load_state_dict on the model or ANY sub-module and .to() / .float() / ... (``_apply``) flag the plan's operands
        as stale immediately; see _weights_changed for everything else."""
        if self.__dict__.get("_dirty_hooks"):
            return
        for m in self.modules():
            m.register_load_state_dict_post_hook(lambda mod, keys, net=self: net._mark_weights_dirty())
        self.__dict__["_dirty_hooks"] = True

    def _apply(self, fn, *args, **kwargs):
        self._mark_weights_dirty()
        return super()._apply(fn, *args, **kwargs)

    def _weight_slots(self):
        """Where every parameter / buffer / sub-module of the WHOLE model lives, with each tensor's identity, storage pointer
        and version counter at the time the plan's operands were folded (``_Folded._snapshot``, which the per-module operand
        caches take of their own tensors).  Walking the module tree costs ~0.65 ms per call; re-reading these ~240 + ~140 dict
        slots costs ~0.06 ms, so _weights_changed can afford to be exact on every cycle."""
        return self._snapshot([self])

    def _weights_changed(self) -> bool:
        """Staleness check of the native plan's operands, once per cycle, EXACT and immediate for every way the weights
        can change: load_state_dict / .to() (dirty flag set by hooks), a replaced Parameter or buffer
        (``net.fc.weight = nn.Parameter(..)``: the slot holds another object), a swapped, added or removed sub-module
        (``net.layers.layer3.tcn.bn = ...``: the ``_modules`` slot holds another object / the dict changed size), an
        in-place edit (``p.add_(..)``: version counter) and ``p.data = ...`` (storage pointer)."""
        return self.__dict__.pop("_weights_dirty", False) or self._stale(self._plan_keep[1])

    def refold(self):
        super().refold()
        self._mark_weights_dirty()

    def _layer_structs(self, device):
        """(ctypes array of csk_co_layer, objects to keep alive, model-level operands): one ``_layer_struct`` per block, plus
        what only the model has -- the adjacency scratch of adaptive graph convs, data_bn and the classifier."""
        arr, keep = (native.CoLayer * 10)(), []
        for i, blk in enumerate(self._blocks):
            arr[i], held = blk._layer_struct(device)
            keep += held
            if not is_plain_graph_conv(blk.gcn):           # adaptive graph conv: adjacency per skeleton frame (agcn.py)
                L, a, dev = arr[i], blk.gcn.plan_operands(device), blk._state.y.device
                adj = self.__dict__.get("_agcn_adj")
                need = self.max_cycle * self._n * self.input_shape[3] * 3 * self.input_shape[2] ** 2      # [cycle frames][skeletons][3][V][V]
                if adj is None or adj.numel() < need or adj.device != dev:
                    adj = self.__dict__["_agcn_adj"] = torch.empty((need,), device=dev, dtype=torch.float32)
                L.agcn_inter, L.agcn_adj_frames = a["inter"], self.max_cycle
                L.agcn_w_pairs, L.agcn_b_pairs, L.agcn_a_sum = a["w_pairs"].data_ptr(), a["b_pairs"].data_ptr(), a["a_sum"].data_ptr()
                L.agcn_adj = adj.data_ptr()
                L.ell_val = None
        ops = self._packed_ops(device)
        fcw, fcb = self.fc.weight.detach(), self.fc.bias.detach()
        keep += [ops, fcw, fcb]
        return arr, keep, ops, fcw, fcb

    def _build_plan(self, device):
        """csk_co_plan (include/cskel.h): one C call per cycle instead of ~25 (CoAGCN: ~45) ctypes calls.  Built for stacks of
        plain GraphConvolution blocks and of adaptive graph convs in the shapes the fused embedding + attention entry
        covers (``plan_operands``); other graph convs keep the Python engine below.  No plan is built while any block has a
        step precision other than "f32" (set_step_precision): ``csk_co_layer`` carries no split weight images, so that mode
        runs on the Python engine (``_python_cycle``); plan support would change the struct and is out of scope."""
        self._destroy_plan()
        if not self.use_native_plan or any(blk.step_precision != "f32" for blk in self._blocks):
            return
        for gcn in (blk.gcn for blk in self._blocks):
            if not is_plain_graph_conv(gcn) and (getattr(gcn, "plan_operands", None) is None or gcn.plan_operands(device) is None):
                return
        c, _, v, m = self.input_shape
        arr, keep, ops, fcw, fcb = self._layer_structs(device)
        plan = native.lib().csk_co_plan_create(10, ctypes.byref(arr), native.ptr(self._xin0), self._xin0.shape[0], self._n, c, v, m, self._p,
                                               native.ptr(ops["scale"]), native.ptr(ops["shift"]), self.num_classes,
                                               native.ptr(fcw), native.ptr(fcb), self.pool_size, self.pool_padding,
                                               native.ptr(self._pool_ring), native.ptr(self._pooled))
        if not plan:
            raise RuntimeError("csk_co_plan_create: " + native.lib().csk_last_error().decode())
        self.__dict__["_plan"] = plan
        delays = (ctypes.c_int32 * 10)(*[blk.delay for blk in self._blocks])      # 4 per block (CoStGcn), 8 (CoStGcnMod)
        native.check(native.lib().csk_co_plan_set_delays(plan, 10, ctypes.byref(delays)), "csk_co_plan_set_delays")
        self._install_dirty_hooks()
        self.__dict__["_plan_keep"] = (keep, self._weight_slots())
        self.__dict__.pop("_weights_dirty", None)
        fuse = all(blk.fuse_step for blk in self._blocks)
        native.check(native.lib().csk_co_plan_set_fusion(plan, int(fuse)), "csk_co_plan_set_fusion")

    def _refresh_plan_weights(self, device):
        """Weights were reloaded / edited in place: refold and hand the new operands to the plan; the
        continual state and its counters are untouched (same semantics as the reference, where weights and
        state buffers are independent)."""
        arr, keep, ops, fcw, fcb = self._layer_structs(device)
        rc = native.lib().csk_co_plan_update_weights(self._plan, 10, ctypes.byref(arr), native.ptr(ops["scale"]),
                                                     native.ptr(ops["shift"]), native.ptr(fcw), native.ptr(fcb))
        native.check(rc, "csk_co_plan_update_weights")
        self.__dict__["_plan_keep"] = (keep, self._weight_slots())

    def _destroy_plan(self):
        plan = self.__dict__.pop("_plan", None)
        if plan:
            native.lib().csk_co_plan_destroy(plan)
        self.__dict__.pop("_plan_keep", None)

    def __del__(self):
        try:
            self._destroy_plan()
        except Exception:
            pass

    def _plan_cycle(self, frames):
        if self._weights_changed():
            self._refresh_plan_weights(frames[0].device)
        n = frames[0].shape[0]
        ptrs = (ctypes.c_void_p * len(frames))(*[x_t.data_ptr() for x_t in frames])
        logits = torch.empty((native.CO_MAX_CYCLE, n, self.num_classes), device=frames[0].device, dtype=torch.float32)
        slot, nf, nl = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        rc = native.lib().csk_co_plan_cycle(self._plan, self._ctr, 22, ptrs, len(frames), native.ptr(logits), ctypes.byref(slot),
                                            ctypes.byref(nf), ctypes.byref(nl), native.stream_of(frames[0]))
        native.check(rc, "csk_co_plan_cycle")      # a failed cycle leaves the counters as they were (include/cskel.h)
        if nf.value == 0:
            return None, 0, []
        return slot.value, nf.value, [logits[j] for j in range(nl.value)]
