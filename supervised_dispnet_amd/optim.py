"""Flat parameter arena + fused Adam and SGD (reference: torch.optim.Adam at train.py:303-305,520-522, torch.optim.SGD at train.py:300-301).

ParamArena (device-agnostic, pure plumbing): re-points every hot parameter at a slice of ONE fp32 buffer and gives each a
gradient view into a second one (`param._dn_grad_view`), ordered by the order gradients are PRODUCED in backward, so
the data-parallel reducer can all-reduce contiguous buckets as soon as they are complete.
FusedAdam (HIP): one `dn_adam_step` launch over the whole arena; numerics follow torch.optim.Adam (amsgrad off):
lerp / addcmul updates, denom = sqrt(v)/sqrt(1-b2^t) + eps, step_size = lr/(1-b1^t); grad * (1/world) folded in.
FusedSGD (HIP): the same surface over the same arena with one `dn_sgd_step` launch; numerics follow torch.optim.SGD with momentum
(dampening 0, nesterov off): buf = momentum*buf + (g + wd*p), p -= lr*buf, the buffer starting as zeros.
Parameter groups (torch-style `[{"params": ..., "lr": ...}, ...]`; only lr may differ): the arena keeps its production order, records each
slice's group and the runs of equal group, and FusedSGD updates any range with one `dn_sgd_step_groups` launch.
"""
import torch

from . import _lib, engine


def split_param_groups(params):
    """What the arena and the optimizers are constructed from -- a flat parameter list or torch-style groups -- as (the parameters in
    construction order, the group of each, one dict of the options besides "params" per group).  Construction order is what a
    torch.optim state dict indexes.  Only "lr" may differ between groups: a parameter listed twice, or another key set to two different
    values, is a ValueError.  Pure bookkeeping, no device."""
    params = list(params)
    if not params or not isinstance(params[0], dict):
        return params, [0] * len(params), [{}]
    listed, group_of, options, seen = [], [], [], set()
    for gi, g in enumerate(params):
        if not isinstance(g, dict) or "params" not in g:
            raise ValueError("parameter group %d is not a dict with a 'params' entry" % gi)
        ps = [g["params"]] if isinstance(g["params"], torch.Tensor) else list(g["params"])
        for p in ps:
            if id(p) in seen:
                raise ValueError("a parameter of group %d appears in more than one parameter group (or twice in one)" % gi)
            seen.add(id(p))
        listed += ps
        group_of += [gi] * len(ps)
        options.append({k: v for k, v in g.items() if k != "params"})
    for key in sorted({k for o in options for k in o if k != "lr"}):
        values = [o[key] for o in options if key in o]
        if any(v != values[0] for v in values):
            raise ValueError("parameter groups set %s to %s: only lr may differ between the groups of one arena" % (key, values))
    return listed, group_of, options


def group_runs(offsets, total, group_of):
    """The runs of equal group over an arena: [(end offset in elements, group)], ends ascending, the last one `total`.  A slice reaches
    to the next slice's offset, so its padding belongs to its group."""
    runs = []
    for i, g in enumerate(group_of):
        end = offsets[i + 1] if i + 1 < len(offsets) else total
        if runs and runs[-1][1] == g:
            runs[-1] = (end, g)
        else:
            runs.append((end, g))
    return runs


class ParamArena(object):
    def __init__(self, params, production_order=None):
        self.listed, listed_group, self.group_options = split_param_groups(params)
        self.listed_group = listed_group                 # group of listed[i]; listed = construction order, frozen parameters included
        group = {id(p): g for p, g in zip(self.listed, listed_group)}
        params = [p for p in self.listed if p.requires_grad]
        if not params:
            raise ValueError("ParamArena got no trainable parameters")
        if production_order is not None:
            rank = {id(p): i for i, p in enumerate(production_order)}
            params = sorted(params, key=lambda p: rank.get(id(p), len(rank)))
            if len(self.group_options) > 1:
                missed = sum(1 for p in production_order if p.requires_grad and id(p) not in group)
                if missed:
                    raise ValueError("the parameter groups miss %d trainable parameter(s) of the production order" % missed)
        self.params = params
        dev = params[0].device
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4        # 16-byte aligned slices
        self.numel, self.offsets = total, offs
        self.n_groups = len(self.group_options)
        self.group_of = [group[id(p)] for p in params]       # per slice, in arena (= gradient production) order
        self.runs = group_runs(offs, total, self.group_of)
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(params, offs):
                view = self.flat_p[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p._dn_grad_view = self.flat_g[o:o + p.numel()].view(p.shape)
        engine.bump_param_epoch()

    def gather_stray_grads(self):
        """Parameters whose gradient arrived through autograd (.grad) instead of the engine's in-place sink."""
        for p in self.params:
            if p.grad is not None:
                p._dn_grad_view.copy_(p.grad)
                p.grad = None


class _ArenaOptimizer(object):
    """What the fused optimizers share: the arena, stray-gradient bookkeeping and the per-bucket overlap contract."""
    arena = None
    _overlap = None           # overlap_backward(): the bucket watcher that applies ranges of the update as their gradients complete

    @property
    def params(self):
        return self.arena.params

    def zero_grad(self, set_to_none=True):
        # arena gradients are fully overwritten by the engine every backward; only stray autograd grads need clearing
        for p in self.arena.params:
            p.grad = None

    def overlap_backward(self, reducer):
        """Apply the update a gradient bucket at a time, as soon as the bucket's gradients (and, under data parallelism, their
        all-reduce) are complete, on a stream of its own under the rest of the backward pass (distributed.GradReducer drives it; with
        one rank the reducer exchanges nothing and only watches the buckets).  Element-wise arithmetic: bit-identical to one update
        of the whole arena.  What is left at step() is bookkeeping; the unoverlappable tail of a step shrinks from the whole
        arena's 0.09 ms pass to the last ~1 MB bucket's.  Contract: exactly one backward pass per step(), through the engine (no
        gradient accumulation, no stray autograd .grad on the arena's parameters)."""
        self._overlap = reducer
        if reducer is not None:
            reducer.optimizer = self
        return self

    def _take_overlapped_step(self):
        """step() under overlap_backward: every range was applied as its bucket completed (GradReducer.finish() has applied the
        stragglers and joined the stream); check the contract."""
        who = type(self).__name__
        if not self._overlap.take_step_applied():
            raise RuntimeError(who + ".overlap_backward: step() without a backward pass + GradReducer.finish() before it")
        if any(p.grad is not None for p in self.arena.params):
            raise RuntimeError(who + ".overlap_backward: a parameter received its gradient through autograd (.grad), not the engine")


class FusedAdam(_ArenaOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, production_order=None):
        if not isinstance(params, ParamArena):
            params = list(params)
        if (params.n_groups if isinstance(params, ParamArena) else len(split_param_groups(params)[2])) > 1:
            # (the reference's grouped recipe, --diff-lr, is SGD; there is no grouped Adam kernel and nothing falls back to a loop of launches)
            raise ValueError("FusedAdam takes one parameter group; per-group learning rates are FusedSGD's (dn_sgd_step_groups)")
        self.arena = params if isinstance(params, ParamArena) else ParamArena(params, production_order)
        engine.require_cuda(self.arena.flat_p, "parameters")
        lr = self.arena.group_options[0].get("lr", lr)
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.step_count = 0
        self.exp_avg = torch.zeros_like(self.arena.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.arena.flat_p)
        self.param_groups = [{"params": self.arena.params, "lr": self.lr, "betas": self.betas, "eps": self.eps,
                              "weight_decay": self.weight_decay}]
        self._dev = None          # capturable(): device-resident step counter / hyper-parameters for hipGraph replay
        self._overlap = None      # overlap_backward(): the bucket watcher that applies ranges of the update as their gradients complete

    def capturable(self, on=True):
        """Keep the step counter and (lr, beta1, beta2) on the DEVICE (dn_adam_step_dev) so that a captured hipGraph of the
        training step advances the bias corrections on every replay; a scheduler changes lr through set_lr()."""
        if on and self._dev is None:
            dev = self.arena.flat_p.device
            g = self.param_groups[0]
            self._dev = {"hyper": torch.tensor([float(g["lr"]), self.betas[0], self.betas[1]], dtype=torch.float64, device=dev),
                         "step": torch.tensor([self.step_count], dtype=torch.int32, device=dev),
                         "derived": torch.zeros(4, dtype=torch.float32, device=dev), "lr": float(g["lr"])}
        elif not on and self._dev is not None:
            self.step_count = int(self._dev["step"].item())
            self._dev = None
        return self

    def set_lr(self, lr):
        self.param_groups[0]["lr"] = float(lr)
        if self._dev is not None and self._dev["lr"] != float(lr):
            self._dev["hyper"][0:1].fill_(float(lr))
            self._dev["lr"] = float(lr)

    @torch.no_grad()
    def apply_range(self, lo, hi, grad_scale=1.0, tick=True):
        """Adam update of arena elements [lo, hi) on the current stream (engine.stream_scope); `tick`: this is the first range of the
        optimizer step (the device-side counter and bias corrections advance once per step)."""
        a = self.arena
        g = self.param_groups[0]
        n = hi - lo
        ptr = lambda t: t.data_ptr() + 4 * lo
        if self._dev is not None:
            d = self._dev
            if d["lr"] != float(g["lr"]):
                self.set_lr(g["lr"])
            if tick:
                _lib.call("dn_adam_tick", d["hyper"].data_ptr(), d["step"].data_ptr(), d["derived"].data_ptr(), engine._stream())
            engine.hbm_call("dn::adam_dev_kernel", n * 28, "dn_adam_step_dev", ptr(a.flat_p), ptr(a.flat_g), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                            n, d["hyper"].data_ptr(), self.eps, self.weight_decay, None, d["derived"].data_ptr(), float(grad_scale), engine._stream())
        else:
            engine.hbm_call("dn::adam_kernel", n * 28, "dn_adam_step", ptr(a.flat_p), ptr(a.flat_g), ptr(self.exp_avg), ptr(self.exp_avg_sq), n,
                            float(g["lr"]), self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count + 1, float(grad_scale),
                            engine._stream())

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        a = self.arena
        if self._overlap is not None:
            self._take_overlapped_step()
            self.step_count += 1
            engine.bump_param_epoch()
            return
        a.gather_stray_grads()
        self.step_count += 1
        g = self.param_groups[0]
        if self._dev is not None:
            d = self._dev
            if d["lr"] != float(g["lr"]):
                self.set_lr(g["lr"])
            engine.hbm_call("dn::adam_dev_kernel", a.numel * 28, "dn_adam_step_dev", a.flat_p.data_ptr(), a.flat_g.data_ptr(),
                            self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), a.numel, d["hyper"].data_ptr(), self.eps,
                            self.weight_decay, d["step"].data_ptr(), d["derived"].data_ptr(), float(grad_scale), engine._stream())
            engine.bump_param_epoch()
            return
        engine.hbm_call("dn::adam_kernel", a.numel * 28, "dn_adam_step", a.flat_p.data_ptr(), a.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                  self.exp_avg_sq.data_ptr(), a.numel, float(g["lr"]), self.betas[0], self.betas[1], self.eps,
                  self.weight_decay, self.step_count, float(grad_scale), engine._stream())
        engine.bump_param_epoch()

    def tape_state(self):
        """The device tensors a replay check must compare (graph.TapedStep.verify); needs capturable(True)."""
        return [self.arena.flat_p, self.exp_avg, self.exp_avg_sq, self._dev["step"], self._dev["derived"]]

    def state_dict(self):
        if self._dev is not None:
            self.step_count = int(self._dev["step"].item())
        return {"step": self.step_count, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"}]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        if self._dev is not None:
            self._dev["step"].fill_(self.step_count)
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])


def flat_momentum_from_torch_sgd(sd, params, arena):
    """A torch.optim.SGD state dict (what --sgd runs wrote before FusedSGD existed, and what the reference writes) as one flat
    momentum buffer in `arena`'s layout, on the CPU.  state[i] belongs to params[i], the list the optimizer was constructed from (the
    arena orders its slices by gradient production instead).  A parameter without an entry never had a gradient: zeros, like the
    padding behind odd-sized slices.  Needs no GPU."""
    params = list(params)
    state, groups = sd["state"], sd.get("param_groups", [])
    count = sum(len(g["params"]) for g in groups) if groups else len(params)
    if count != len(params):
        raise ValueError("torch.optim.SGD state for %d parameters, this optimizer was built from %d" % (count, len(params)))
    offset = {id(p): o for p, o in zip(arena.params, arena.offsets)}
    flat = torch.zeros(arena.numel, dtype=torch.float32)
    for i, entry in state.items():
        i = int(i)
        if not 0 <= i < len(params):
            raise ValueError("torch.optim.SGD state has an entry for parameter %d of %d" % (i, len(params)))
        buf = entry.get("momentum_buffer")
        o = offset.get(id(params[i]))
        if buf is None or o is None:          # (momentum 0 leaves None; a frozen parameter is not in the arena)
            continue
        if tuple(buf.shape) != tuple(params[i].shape):
            raise ValueError("torch.optim.SGD momentum_buffer of parameter %d has shape %s, the parameter %s"
                             % (i, tuple(buf.shape), tuple(params[i].shape)))
        flat[o:o + buf.numel()] = buf.detach().reshape(-1).to("cpu", torch.float32)
    return flat


def grouped_state(param_groups, listed_group):
    """state_dict()["param_groups"] of a grouped optimizer, as torch writes it: each group's hyper-parameters plus "params", the indices of
    its parameters in the construction-order list (listed_group[i] = the group of parameter i)."""
    return [dict({k: v for k, v in g.items() if k != "params"}, params=[i for i, gg in enumerate(listed_group) if gg == gi])
            for gi, g in enumerate(param_groups)]


def require_same_grouping(sd, sizes):
    """ValueError unless the state dict's param_groups list as many parameters, group by group, as `sizes`."""
    got = [len(g["params"]) if "params" in g else None for g in sd.get("param_groups", [])]
    if got != list(sizes):
        raise ValueError("optimizer state for parameter groups of sizes %s, this optimizer has groups of sizes %s" % (got, list(sizes)))


class FusedSGD(_ArenaOptimizer):
    """torch.optim.SGD with momentum (dampening 0, nesterov off) as one dn_sgd_step launch over the arena: FusedAdam's surface, so
    distributed.GradReducer, graph.TapedStep / GraphedStep and train.py take either.  The momentum buffer starts as zeros, which is the
    gradient copy torch's first step makes (momentum*0 + g), so there is no step counter: any range of the arena is one launch and
    apply_range's `tick` has nothing to do."""

    def __init__(self, params, lr=None, momentum=0.0, weight_decay=0.0, production_order=None):
        hyper = {"momentum": float(momentum), "weight_decay": float(weight_decay), "dampening": 0, "nesterov": False}
        if isinstance(params, ParamArena):
            options = params.group_options
        else:
            params = list(params)
            options = split_param_groups(params)[2]
        for gi, o in enumerate(options):          # (before the arena re-points a single parameter)
            for k, v in o.items():
                if k != "lr" and (k not in hyper or v != hyper[k]):
                    raise ValueError("FusedSGD: parameter group %d sets %s=%r, the optimizer has %r: only lr may differ between groups"
                                     % (gi, k, v, hyper.get(k, "no such option")))
            if "lr" not in o and lr is None:
                raise ValueError("FusedSGD: no learning rate for parameter group %d" % gi)
        if isinstance(params, ParamArena):
            self.arena = params
            # (one group: a torch.optim.SGD state dict indexes the arena's own list, as it always has for a ready-made arena)
            self._listed = list(params.params) if params.n_groups == 1 else list(params.listed)
        else:
            self.arena = ParamArena(params, production_order)
            self._listed = list(self.arena.listed)       # construction order: the index of a torch.optim.SGD state dict
        engine.require_cuda(self.arena.flat_p, "parameters")
        a = self.arena
        self.weight_decay = float(weight_decay)
        self.momentum_buffer = torch.zeros_like(a.flat_p)
        rates = [float(o.get("lr", lr)) for o in options]
        self._dev = None          # capturable(): device-resident (lr, momentum) for a captured or taped step
        self._table = None        # several groups: the run table and the rates, on the device in every mode (dn_sgd_step_groups)
        self._overlap = None
        if a.n_groups == 1:
            self.param_groups = [{"params": a.params, "lr": rates[0], "momentum": float(momentum), "weight_decay": self.weight_decay,
                                  "dampening": 0, "nesterov": False}]
            return
        self.param_groups = [{"params": [p for p, g in zip(a.listed, a.listed_group) if g == gi], "lr": rates[gi], "momentum": float(momentum),
                              "weight_decay": self.weight_decay, "dampening": 0, "nesterov": False} for gi in range(a.n_groups)]
        dev = a.flat_p.device
        self._table = {"seg_end": torch.tensor([e for e, _ in a.runs], dtype=torch.int64, device=dev),
                       "seg_group": torch.tensor([g for _, g in a.runs], dtype=torch.int32, device=dev),
                       "lr": torch.tensor(rates, dtype=torch.float64, device=dev), "host": list(rates)}

    def capturable(self, on=True):
        """Keep (lr, momentum) on the DEVICE (dn_sgd_step_dev) so that a captured step follows a scheduler: set_lr() writes the value.
        With several groups the rates are on the device in every mode and there is nothing to move."""
        if self._table is not None:
            return self
        if on and self._dev is None:
            g = self.param_groups[0]
            self._dev = {"hyper": torch.tensor([float(g["lr"]), float(g["momentum"])], dtype=torch.float64, device=self.arena.flat_p.device),
                         "lr": float(g["lr"])}
        elif not on:
            self._dev = None
        return self

    def set_lr(self, lr, group=0):
        self.param_groups[group]["lr"] = float(lr)
        if self._table is not None:
            if self._table["host"][group] != float(lr):
                self._table["lr"][group:group + 1].fill_(float(lr))
                self._table["host"][group] = float(lr)
        elif self._dev is not None and self._dev["lr"] != float(lr):
            self._dev["hyper"][0:1].fill_(float(lr))
            self._dev["lr"] = float(lr)

    @torch.no_grad()
    def apply_range(self, lo, hi, grad_scale=1.0, tick=True):
        """SGD update of arena elements [lo, hi) on the current stream (engine.stream_scope).  `tick` is FusedAdam's once-per-step
        advance of its counter; SGD has no per-step state, so it is accepted and unused.  Several groups: one dn_sgd_step_groups launch
        over the arena bases and the range, whatever runs the range cuts through."""
        a, g = self.arena, self.param_groups[0]
        n = hi - lo
        if self._table is not None:
            t = self._table
            for gi, grp in enumerate(self.param_groups):
                if t["host"][gi] != float(grp["lr"]):
                    self.set_lr(grp["lr"], gi)
            engine.hbm_call("dn::sgd_groups_kernel", n * 20, "dn_sgd_step_groups", a.flat_p.data_ptr(), a.flat_g.data_ptr(),
                            self.momentum_buffer.data_ptr(), lo, hi, t["seg_end"].data_ptr(), t["seg_group"].data_ptr(), len(a.runs),
                            t["lr"].data_ptr(), a.n_groups, float(g["momentum"]), self.weight_decay, float(grad_scale), engine._stream())
            return
        ptr = lambda t: t.data_ptr() + 4 * lo
        if self._dev is not None:
            if self._dev["lr"] != float(g["lr"]):
                self.set_lr(g["lr"])
            engine.hbm_call("dn::sgd_dev_kernel", n * 20, "dn_sgd_step_dev", ptr(a.flat_p), ptr(a.flat_g), ptr(self.momentum_buffer), n,
                            self._dev["hyper"].data_ptr(), self.weight_decay, float(grad_scale), engine._stream())
        else:
            engine.hbm_call("dn::sgd_kernel", n * 20, "dn_sgd_step", ptr(a.flat_p), ptr(a.flat_g), ptr(self.momentum_buffer), n,
                            float(g["lr"]), float(g["momentum"]), self.weight_decay, float(grad_scale), engine._stream())

    @torch.no_grad()
    def step(self, grad_scale=1.0):
        if self._overlap is not None:
            self._take_overlapped_step()
        else:
            self.arena.gather_stray_grads()
            self.apply_range(0, self.arena.numel, grad_scale)
        engine.bump_param_epoch()

    def tape_state(self):
        """The device tensors a replay check must compare (graph.TapedStep.verify)."""
        return [self.arena.flat_p, self.momentum_buffer]

    def state_dict(self):
        if len(self.param_groups) == 1:
            groups = [{k: v for k, v in self.param_groups[0].items() if k != "params"}]
        else:
            groups = grouped_state(self.param_groups, self.arena.listed_group)
        return {"momentum_buffer": self.momentum_buffer.clone(), "param_groups": groups}

    def load_state_dict(self, sd):
        """This class's own form, or a torch.optim.SGD state dict over the parameter list (or groups) this optimizer was constructed from.
        The state is the momentum buffer; the rates stay what the constructor or set_lr made them."""
        if len(self.param_groups) > 1 or len(sd.get("param_groups", [])) > 1:
            require_same_grouping(sd, [len(g["params"]) for g in self.param_groups] if len(self.param_groups) > 1 else [len(self._listed)])
        if "momentum_buffer" in sd:
            flat = sd["momentum_buffer"]
            if flat.numel() != self.arena.numel:
                raise ValueError("momentum_buffer of %d elements, the arena has %d" % (flat.numel(), self.arena.numel))
        elif "state" in sd:
            flat = flat_momentum_from_torch_sgd(sd, self._listed, self.arena)
        else:
            raise ValueError("neither a FusedSGD nor a torch.optim.SGD state dict (keys: %s)" % sorted(sd))
        self.momentum_buffer.copy_(flat.reshape(-1))
