"""SceneAdaptiveInterpolation: the MAML / MAML++ / Meta-SGD / L2F system around a VFI plugin.

Drop-in for the reference class of the same name (meta_learning_system.py:29-697): same constructor
(``SceneAdaptiveInterpolation(args)``), same methods called by ExperimentBuilder
(``run_train_iter / run_validation_iter / run_test_iter``), same attributes (``optimizer``,
``scheduler``, ``net``, ``inner_loop_optimizer``, ``attenuator``, ``gamma_mult``, ``mean``/``std``) and
the same ``state_dict`` key layout.  Per task and inner step: two support passes ((0,4)->2 and
(2,6)->4), one ``autograd.grad`` over both, one per-parameter update; then the target pass (2,4)->3.

What is different (MI355X-first, results identical):
  * model ops and the update are HIP kernels behind the C ABI (sepconv, voxel warp, pixel shuffle,
    fused multi-tensor update, L2F mean/scale, fused L1/MSE);
  * the two support triplets of a step -- same weights, independent samples -- run as one N=2 forward
    (``--fuse_support_pairs 0`` restores two N=1 calls);
  * no host synchronisation inside the task loop: the reference pulls every loss to the host
    (:332) and every ``zero_grad(params)`` syncs per parameter; here loss scalars stay on the device
    and are fetched once per iteration;
  * tasks shard across processes (task_parallel.TaskParallel) with one all-reduce of outer grads;
    with a single process this is the reference's sequential loop.  The reference's ``.module`` call
    for >1 visible device (:285-287) is not reproduced: one process owns one device.
"""
import contextlib
import functools
import gc
import os
import threading

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from . import _hip, graph_inner_loop, hip_ops, model_utils, utils
from .inner_loop_optimizers import LSLRGradientDescentLearningRule, MetaSGDLearningRule
from .loss import CharbonnierLoss, Loss
from .task_parallel import TaskParallel
from .task_schedule import autograd_mode, target_schedule, task_picker


def set_torch_seed(seed):
    """Seed torch from a numpy stream, returning that stream (reference :16-26)."""
    rng = np.random.RandomState(seed=seed)
    torch.manual_seed(seed=int(rng.randint(0, 999999)))
    return rng


# ---------------------------------------------------------------------------------------------
# --model plugin surface
# ---------------------------------------------------------------------------------------------
def _build_sepconv(args, resume):
    from .sepconv.model import MetaNetwork
    return MetaNetwork(resume=resume, strModel='l1', windowed=bool(getattr(args, 'sepconv_window', 1)))


def _build_cain(args, resume):
    from .cain.model import MetaCAIN
    return MetaCAIN(depth=3, resume=resume)


def _build_voxelflow(args, resume):
    from .voxelflow.core.models.voxel_flow import MetaVoxelFlow
    return MetaVoxelFlow(args, resume=resume)


def _build_rrin(args, resume):
    from .rrin.model import MetaRRIN
    return MetaRRIN(level=3, resume=resume)


def _build_superslomo(args, resume):
    from .superslomo.model import MetaSuperSloMo
    return MetaSuperSloMo(torch.device('cuda') if args.cuda else torch.device('cpu'), resume=resume)


def _build_dain(args, resume):
    from .dain.networks.DAIN import MetaDAIN
    return MetaDAIN(resume=resume)


def _build_adacof(args, resume):
    from .adacof.model import MetaAdaCoF
    return MetaAdaCoF(kernel_size=int(getattr(args, 'adacof_kernel_size', 5)), dilation=int(getattr(args, 'adacof_dilation', 1)),
                      resume=resume)


def _build_softsplat(args, resume):
    from .softsplat.model import MetaSoftSplat
    return MetaSoftSplat(alpha=float(getattr(args, 'softsplat_alpha', -20.0)), mode=str(getattr(args, 'softsplat_mode', 'soft')), resume=resume)


MODEL_REGISTRY = {'sepconv': _build_sepconv, 'cain': _build_cain, 'voxelflow': _build_voxelflow, 'rrin': _build_rrin,
                  'superslomo': _build_superslomo, 'dain': _build_dain, 'adacof': _build_adacof, 'softsplat': _build_softsplat}


def register_model(name, factory):
    """Add a ``--model`` plugin: ``factory(args, resume) -> nn.Module`` with
    ``forward(frame0, frame1, params=None, **kw)``, ``zero_grad(params)``, ``restore_backup_stats()``."""
    MODEL_REGISTRY[name] = factory


class _DeferredMeters:
    """Collects device scalars during the task loop; turns them into AverageMeters with ONE sync."""

    def __init__(self):
        self.items = {}

    def add(self, key, value):
        self.items.setdefault(key, []).append(value.detach())

    def flush(self):
        meters = {}
        if not self.items:
            return meters
        keys = list(self.items)
        flat = torch.stack([v.reshape(()) for k in keys for v in self.items[k]]).cpu().numpy()
        i = 0
        for k in keys:
            m = utils.AverageMeter()
            for _ in self.items[k]:
                m.update(flat[i])
                i += 1
            meters[k] = m
        return meters


class _LazyLog(dict):
    """The dict run_train_iter returns (`losses`, `metrics`): what needs the device to have finished -- logged losses, PSNR / SSIM
    meters, the importance vector -- is fetched on the FIRST READ instead of before returning.  A caller that logs every
    iteration (ExperimentBuilder, the reference's loop) syncs exactly where it did; one that does not read (a timing loop)
    lets the host run on into the next iteration while the device finishes this one -- the one host sync per iteration was a
    1-5 ms bubble at every iteration boundary (profiles/r03_*_one_iteration.txt: the largest gap of each trace)."""

    def __init__(self, data, ensure):
        super().__init__(data)
        self._data, self._ensure = data, ensure

    def _ready(self):
        ensure, self._ensure = self._ensure, None
        if ensure is not None:
            ensure()
            dict.update(self, self._data)

    def __reduce__(self):            # pickle / torch.save / copy.deepcopy: a plain dict of the finished values
        self._ready()
        return (dict, (dict(self),))


def _lazy_forward(name):
    plain = getattr(dict, name)

    def method(self, *a, **kw):
        self._ready()
        return plain(self, *a, **kw)
    method.__name__ = name
    return method


# every accessor and mutator of dict goes through _ready() first: a partly overridden dict subclass would let copy(), pop(),
# ==, | ... see the dict as it was before the device finished
for _name in ('__getitem__', '__setitem__', '__delitem__', '__contains__', '__iter__', '__len__', '__repr__', '__eq__', '__ne__',
              '__or__', '__ror__', '__ior__', '__reversed__', 'get', 'keys', 'values', 'items', 'copy', 'pop', 'popitem',
              'setdefault', 'update', 'clear'):
    setattr(_LazyLog, _name, _lazy_forward(_name))
del _name


class SceneAdaptiveInterpolation(nn.Module):
    MAX_GRAPH_SETS = 8

    def __init__(self, args, net=None, inner_loop_optimizer=None, criterion=None, task_parallel=None):
        super().__init__()
        self.args = args
        self.device = torch.device('cuda') if args.cuda else torch.device('cpu')
        self.batch_size = args.batch_size
        self.use_cuda = args.cuda
        self.current_epoch = 0
        self.fuse_support_pairs = bool(getattr(args, 'fuse_support_pairs', 1))

        # 7-frame septuplets: supports (0,4)->2 and (2,6)->4, target (2,4)->3; 4-frame clips at test time
        self.support_idxs = [[0, 1, 2], [1, 2, 3]] if args.mode == 'test' else [[0, 2, 4], [2, 4, 6]]
        self.target_idxs = [2, 3, 4]

        self.rng = set_torch_seed(seed=args.random_seed)
        if net is not None:
            self.net = net.to(self.device)
        else:
            if args.model == 'dain' and not args.cuda:
                raise NotImplementedError("Model not implemented on the host! DAIN's two own ops (dain/my_package: "
                                          "FilterInterpolationModule, DepthFlowProjectionModule), its flow estimator "
                                          "(dain/PWCNet: PWCDCNet, Correlation) and the rest of the MetaDAIN plugin run on the HIP "
                                          "kernels only: --model dain has no CPU path.")
            if args.model not in MODEL_REGISTRY:
                raise NotImplementedError('Model not implemented yet!')
            print('Building %s model...' % args.model)
            self.net = MODEL_REGISTRY[args.model](args, not args.resume).to(self.device)
        if int(getattr(args, 'dain_task_modes', 0) or 0) and hasattr(self.net, 'alloc_front'):
            # --dain_task_modes 1: THIS MetaDAIN instance takes the lockstep and hipGraph paths (its class declines both)
            self.net.lockstep_tasks = True
            self.net.graph_capture = True
        if hasattr(self.net, 'sepconv_second_order'):
            # --sepconv_second_order 1: THIS SepConv plugin carries the second-order terms through its 51-tap op (second-order passes only)
            self.net.sepconv_second_order = bool(int(getattr(args, 'sepconv_second_order', 0) or 0))
        if args.model == 'voxelflow':
            half = torch.full((3, 1, 1), 0.5 * 255, device=self.device)
            self.mean, self.std = half.clone(), half.clone()
        if args.model == 'superslomo':
            # Super SloMo frames are mean-subtracted by the loaders; revNormalize brings outputs back to 0..1
            # (the reference builds transforms.Normalize(mean=-m, std=1) for this, :69-73)
            shift = torch.tensor([.429, .431, .397], device=self.device).view(3, 1, 1)
            self.revNormalize = lambda img: img + shift

        self.inner_learning_rate = args.inner_lr
        if inner_loop_optimizer is not None:
            self.inner_loop_optimizer = inner_loop_optimizer
        elif args.metasgd:
            print('Adaptation with Meta-SGD')
            self.inner_loop_optimizer = MetaSGDLearningRule(device=self.device, optimizer=args.optimizer,
                                                            init_learning_rate=self.inner_learning_rate)
        else:
            self.inner_loop_optimizer = LSLRGradientDescentLearningRule(
                device=self.device, optimizer=args.optimizer, init_learning_rate=self.inner_learning_rate,
                total_num_inner_loop_steps=args.number_of_training_steps_per_iter,
                use_learnable_learning_rates=args.learnable_per_layer_per_step_inner_loop_learning_rate)

        if hasattr(self.net, 'freeze_front'):
            # dain: everything outside rectifyNet is constant (reference :96-101) -- before the inner-loop dictionary is built
            self.net.freeze_front()
        names_weights = self.get_inner_loop_parameter_dict(self.net.named_parameters())
        self.inner_loop_optimizer.initialize(names_weights_dict=names_weights)

        if args.attenuate:  # L2F: gamma = 1 - gamma_mult * MLP(layer-wise mean grads)
            L = len(names_weights)
            print('# of layers: %d' % L)
            self.attenuator = nn.Sequential(nn.Linear(L, L), nn.ReLU(inplace=True), nn.Linear(L, L),
                                            nn.Sigmoid()).to(self.device)
            self.gamma_mult = nn.Parameter(torch.zeros(1))

        self.to(self.device)

        if args.optimizer == 'Adam':
            if args.model == 'voxelflow' and hasattr(self.net, 'get_optim_policies'):
                self.optimizer = optim.Adam(self.net.get_optim_policies(), lr=args.outer_lr,
                                            weight_decay=args.weight_decay)
            else:
                self.optimizer = optim.Adam(self.trainable_parameters(), lr=args.outer_lr, betas=(0.9, 0.99))
        elif args.optimizer == 'Adamax':
            self.optimizer = optim.Adamax(self.trainable_parameters(), lr=args.outer_lr, betas=(0.9, 0.999))
        else:
            self.optimizer = optim.SGD(self.trainable_parameters(), lr=args.outer_lr)
        self.scheduler = optim.lr_scheduler.ReduceLROnPlateau(optimizer=self.optimizer, mode='min', factor=0.2,
                                                              patience=5)
        print('# of parameters: %d' % sum(p.numel() for p in self.trainable_parameters()))

        if criterion is not None:
            self.criterion = criterion
        elif args.model == 'dain':     # the network's own Charbonnier loss whatever --loss says (reference :493-505)
            self.criterion = CharbonnierLoss()
        else:
            self.criterion = Loss(args)
        self.task_parallel = task_parallel if task_parallel is not None else TaskParallel()
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                _hip.ws_watch()
        self._first_order = False
        self._defer_logging = False
        self._pending_logging = None
        self._filter_modules = None
        self._task_stream_pool = None
        self._routes = None          # (routed, unrouted) inner-loop tensor names, probed once (_routing)
        self._graphs = {}            # (frame shape, steps, training, msl) -> GraphedInnerLoop
        self._manual_grads = None    # OuterGradAccumulator of the last graphed training forward

        if args.resume:
            print('Resume training')
            utils.load_checkpoint(args, self, None)
        if args.pretrained_model is not None:
            print('Loading pretrained model: %s' % args.pretrained_model)
            ckpt = torch.load(args.pretrained_model, map_location='cpu', weights_only=False)
            with torch.no_grad():
                if args.model == 'dain':         # the bare state dict (reference :168-169)
                    utils.lossy_load_state_dict(self.net, ckpt)
                elif 'state_dictFC' in ckpt:     # Super SloMo's released checkpoints (reference :162-167)
                    self.net.flowComp.load_state_dict(ckpt['state_dictFC'])
                    self.net.arbTimeFlowIntrp.load_state_dict(ckpt['state_dictAT'])
                else:
                    utils.lossy_load_state_dict(self.net, ckpt['state_dict'])

    # -----------------------------------------------------------------------------------------
    # small pieces kept with the reference's names
    # -----------------------------------------------------------------------------------------
    def get_per_step_loss_importance_vector(self):
        """MAML++ multi-step-loss weights (reference :186-210): uniform 1/S, non-final entries decay
        with the epoch down to 0.03/S, the final one grows up to 1-(S-1)*0.03/S."""
        S = self.args.number_of_training_steps_per_iter
        # the vector only depends on the epoch: keep the device copy.  A blocking host-to-device copy of a pageable array makes the
        # host wait for everything queued on the stream -- once per forward that was a full host/GPU sync at the top of every
        # meta-iteration (11.7 ms of a 23 ms iteration of config C1 under cProfile: the host could never run ahead of the replays)
        key = (S, self.current_epoch, self.args.multi_step_loss_num_epochs, str(self.device))
        cached = getattr(self, '_importance_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        if S == 0:
            vec = torch.ones(1, device=self.device)
            self._importance_cache = (key, vec)
            return vec
        w = np.ones(shape=(S,)) * (1.0 / S)
        decay = 1.0 / S / self.args.multi_step_loss_num_epochs
        floor = 0.03 / S
        for i in range(S - 1):
            w[i] = np.maximum(w[i] - self.current_epoch * decay, floor)
        w[-1] = np.minimum(w[-1] + self.current_epoch * (S - 1) * decay, 1.0 - (S - 1) * floor)
        vec = torch.Tensor(w).to(device=self.device)
        self._importance_cache = (key, vec)
        return vec

    def get_inner_loop_parameter_dict(self, params):
        """{name: param} of what the inner loop adapts (reference :213-228)."""
        keep_bn = self.args.enable_inner_loop_optimizable_bn_params
        return {name: p for name, p in params if p.requires_grad and (keep_bn or "norm_layer" not in name)}

    def trainable_parameters(self):
        for p in self.parameters():
            if p.requires_grad:
                yield p

    # -----------------------------------------------------------------------------------------
    # forward passes
    # -----------------------------------------------------------------------------------------
    def _front_kw(self, fronts, key, frame0, frame1):
        """A plugin with a frozen front (dain: everything before its rectify net is a function of the frames and of constants)
        evaluates it once per task and triplet and meta-iteration: `fronts` is the task's own {triplet: front}, `key` names the
        triplet.  -> the keyword that hands it to the plugin's forward, or nothing (no such plugin; reuse switched off)."""
        if fronts is None or not getattr(self.net, 'reuse_front', False):
            return {}
        if key not in fronts:
            fronts[key] = self.net.front(frame0, frame1)
        return {'front': fronts[key]}

    @contextlib.contextmanager
    def _pass_flags(self, own_const, overlap):
        """The op layer's two per-pass switches (thread-local there) for the duration of a pass.  own_const: the plugin's own
        parameters, the tensors it does not read from the fast dict, are constants.  overlap: the weight gradients of the pass
        may run beside its data-gradient chain; whoever calls autograd.grad joins them before anything reads them."""
        model_utils.set_own_params_const(own_const)
        hip_ops.set_weight_gradient_overlap(overlap)
        try:
            yield
        finally:
            model_utils.set_own_params_const(False)
            hip_ops.set_weight_gradient_overlap(False)

    def _run_pass(self, frame0, frame1, weights, num_step, *, support, own_const=False, overlap=False, front_kw=None,
                  extras=False, flags=True):
        """THE plugin forward of every task mode: a support pass (which backs up the running statistics at step 0) or a target
        pass on the fast weights -> the frame, with extras=True (frame, Super SloMo's flows and warped frames for its 'Super'
        loss, or None).  flags=False: the caller holds _pass_flags itself, over more than one pass."""
        with self._pass_flags(own_const, overlap) if flags else contextlib.nullcontext():
            out = self.net.forward(frame0, frame1, params=weights, backup_running_statistics=support and num_step == 0,
                                   num_step=num_step, **(front_kw or {}))
        frame, extra = out if isinstance(out, tuple) else (out, None)
        return (frame, extra) if extras else frame

    def _wgrad_overlap(self):
        return self.device.type == 'cuda' and bool(getattr(self.args, 'wgrad_overlap', 0))

    def net_forward(self, frame0, frame1, target, weights, num_step, *, support, front_kw=None, flags=True):
        """One backbone pass with fast weights + criterion -> (losses dict, output)  (reference :475-509)."""
        output, extras = self._run_pass(frame0, frame1, weights, num_step, support=support, front_kw=front_kw, extras=True,
                                        flags=flags)
        if extras is not None:            # superslomo: flows and warped frames for the 'Super' loss  (:499-502)
            return self.criterion(output, target, I0=frame0, I1=frame1, **extras), output
        return self.criterion(output, target), output

    def _support_loss(self, frames, task_id, weights, num_step, fronts=None):
        """Sum of the two support-triplet losses of one inner step (reference :387-396)."""
        a, b = self.support_idxs
        # step 0 differentiates w.r.t. theta itself, whose non-routed tensors ARE the modules' own parameters
        # (reference fact: 94 live tensors at step 0, 54 afterwards); from step 1 on those are constants
        own_const = self._first_order and num_step > 0
        overlap = self._first_order and self._wgrad_overlap()
        if self.fuse_support_pairs:
            sl = slice(task_id, task_id + 1)
            f0 = torch.cat([frames[a[0]][sl], frames[b[0]][sl]], 0)
            f1 = torch.cat([frames[a[2]][sl], frames[b[2]][sl]], 0)
            # superslomo's extras only feed the 'Super' loss, which Loss rejects
            out = self._run_pass(f0, f1, weights, num_step, support=True, own_const=own_const, overlap=overlap,
                                 front_kw=self._front_kw(fronts, 'support', f0, f1))
            return self.criterion(out[0:1], frames[a[1]][sl])['total'] + self.criterion(out[1:2], frames[b[1]][sl])['total']
        total = 0
        with self._pass_flags(own_const, overlap):      # ONE scope: a weight both passes read is counted over both (hip_ops._WG.uses)
            for which, ind in enumerate((a, b)):
                f0, f1 = frames[ind[0]][task_id].unsqueeze(0), frames[ind[2]][task_id].unsqueeze(0)
                losses, _ = self.net_forward(f0, f1, frames[ind[1]][task_id].unsqueeze(0), weights, num_step, support=True,
                                             front_kw=self._front_kw(fronts, 'support%d' % which, f0, f1), flags=False)
                total = total + losses['total']
        return total

    def _target_pass(self, frames, task_id, weights, num_step, fronts=None, with_grad=True):
        t = self.target_idxs
        f0, f1 = frames[t[0]][task_id].unsqueeze(0), frames[t[2]][task_id].unsqueeze(0)
        with autograd_mode(with_grad):
            return self.net_forward(f0, f1, frames[t[1]][task_id].unsqueeze(0), weights, num_step, support=False,
                                    front_kw=self._front_kw(fronts, 'target', f0, f1))

    # -----------------------------------------------------------------------------------------
    # L2F
    # -----------------------------------------------------------------------------------------
    def get_task_embeddings(self, frames, task_id, names_weights_copy, fronts=None):
        """Layer-wise mean of the support gradient at theta (reference :231-255), one fused reduction."""
        loss = self._support_loss(frames, task_id, names_weights_copy, num_step=0, fronts=fronts)
        self.net.zero_grad(names_weights_copy)
        grads = torch.autograd.grad(loss, names_weights_copy.values(), create_graph=False, allow_unused=True)
        hip_ops.join_weight_gradients()
        if any(g is None for g in grads):
            raise AttributeError("L2F needs a gradient for every inner-loop tensor (the reference calls "
                                 ".mean() on None here, meta_learning_system.py:251)")
        return hip_ops.mt_mean(grads)

    def attenuate_init(self, task_embeddings, names_weights_copy):
        """w_i <- gamma_i * w_i with gamma = clamp(1 - gamma_mult * attenuator(e), 0, 1)  (reference :258-272)."""
        gamma = 1 - self.gamma_mult * self.attenuator(task_embeddings)
        gamma.clamp_(0, 1)
        scaled = hip_ops.mt_scale(gamma, list(names_weights_copy.values()))
        return dict(zip(names_weights_copy.keys(), scaled))

    # -----------------------------------------------------------------------------------------
    # inner loop
    # -----------------------------------------------------------------------------------------
    def apply_inner_loop_update(self, loss, names_weights_copy, use_second_order, current_step_idx):
        """grad of the support loss w.r.t. the fast weights, then the learned update (reference :275-321).
        Tensors without a gradient drop out of the dict."""
        self.net.zero_grad(params=names_weights_copy)
        grads = torch.autograd.grad(loss, names_weights_copy.values(), create_graph=use_second_order,
                                    allow_unused=True)
        hip_ops.join_weight_gradients()
        return self.inner_loop_optimizer.update_params(
            names_weights_dict=names_weights_copy,
            names_grads_wrt_params_dict=dict(zip(names_weights_copy.keys(), grads)),
            num_step=current_step_idx)

    def _adapt(self, frames, task_id, num_steps, use_second_order, on_weights=None, fronts=None):
        """Run the inner loop of one task; returns the adapted fast weights.  on_weights(s, W_s) sees the weights after s = 0 ..
        num_steps updates.  fronts: the task's {triplet: front} (_front_kw)."""
        weights = self.get_inner_loop_parameter_dict(self.net.named_parameters())
        weights = {name.replace('module.', ''): v for name, v in weights.items()}
        self.inner_loop_optimizer.initialize_state()
        if self.args.attenuate:
            emb = self.get_task_embeddings(frames, task_id, weights, fronts)
            weights = self.attenuate_init(task_embeddings=emb, names_weights_copy=weights)
        if on_weights is not None:
            on_weights(0, weights)
        for num_step in range(num_steps):
            support_loss = self._support_loss(frames, task_id, weights, num_step, fronts)
            weights = self.apply_inner_loop_update(loss=support_loss, names_weights_copy=weights,
                                                   use_second_order=use_second_order, current_step_idx=num_step)
            if on_weights is not None:
                on_weights(num_step + 1, weights)
        return weights

    def _to_unit_range(self, img):
        if self.args.model == 'voxelflow':
            return (img * self.std + self.mean) / 255.0
        if self.args.model == 'superslomo':
            return self.revNormalize(img)
        return img

    def _eval_metrics(self, preds, targets):
        """preds, targets [rows,C,H,W] in the network's range -> (mse [rows], ssim [rows]) device tensors of the quantised unit-range
        images (reference utils.py:189-204 per pair): one call for all rows, no host read."""
        return utils.psnr_ssim_rows(self._to_unit_range(preds.detach()), self._to_unit_range(targets.detach()))

    def _eval_msssim(self, preds, targets):
        """--eval_msssim 1: the third metric of an evaluated frame, [rows] device values of msssim(quantize(pred), quantize(target),
        val_range=255) (a NaN stays a NaN); None with the default."""
        if not getattr(self.args, 'eval_msssim', 0):
            return None
        return utils.msssim_rows(self._to_unit_range(preds.detach()), self._to_unit_range(targets.detach()))

    def _task_body(self, frames, task_id, *, num_steps, use_second_order, msl, training_phase, do_evaluation, importance):
        """Everything one task contributes to a meta-iteration (reference :366-461): adaptation, target pass(es), its
        loss term, prediction, logging scalars.  Touches no shared mutable state, so tasks can run concurrently."""
        task_losses, logs, state = [], [], {}
        fronts = {} if hasattr(self.net, 'front') else None       # this task's frozen fronts, one per triplet (dain)

        due = {s: (index, with_grad) for s, index, with_grad in target_schedule(num_steps, msl, training_phase)}

        def target(s, weights):
            if s in due:
                index, with_grad = due[s]        # a multi-step-loss pass on W_s is handed num_step = s - 1 (target_schedule)
                tl, state['preds'] = self._target_pass(frames, task_id, weights, s if index is None else s - 1, fronts, with_grad)
                task_losses.append(tl['total'] if index is None else importance[index] * tl['total'])
                logs.extend(tl.items())

        self._adapt(frames, task_id, num_steps, use_second_order, target, fronts)

        target_preds = state['preds']
        res = {'pred': self._to_unit_range(target_preds.detach().squeeze(0)).unsqueeze(0), 'logs': logs}
        if do_evaluation:
            mse, ssim = self._eval_metrics(target_preds, frames[self.target_idxs[1]][task_id:task_id + 1])
            res['mse'], res['ssim'] = mse[0], ssim[0]
            msssim = self._eval_msssim(target_preds, frames[self.target_idxs[1]][task_id:task_id + 1])
            if msssim is not None:
                res['msssim'] = msssim[0]
        res['loss'] = torch.sum(torch.stack(task_losses))
        if not training_phase:
            self.net.restore_backup_stats()
        return res

    # -----------------------------------------------------------------------------------------
    # tasks in lockstep (--task_batch T): the reference's sequential task loop (:366) as ONE pass per inner step
    # -----------------------------------------------------------------------------------------
    def _routing(self, frame_shape):
        """(routed, unrouted) inner-loop tensor names: which of them the plugin actually reads from the fast-weight dict
        (SepConv 54 of 94, VoxelFlow 9 of 23, CAIN 494 of 494: SURVEY.md fact 6).  One eager pass on cloned tensors, once."""
        if self._routes is None:
            theta = self.get_inner_loop_parameter_dict(self.net.named_parameters())
            fast = {k: v.detach().clone().requires_grad_() for k, v in theta.items()}
            x = torch.zeros((1,) + tuple(frame_shape), device=self.device)
            out = self._run_pass(x, x, fast, 0, support=False, front_kw=self._probe_kw(frame_shape))
            g = torch.autograd.grad(out.sum(), list(fast.values()), allow_unused=True)
            self._routes = ([k for k, gi in zip(fast, g) if gi is not None], [k for k, gi in zip(fast, g) if gi is None])
        return self._routes

    def _probe_kw(self, frame_shape):
        """A plugin with a frozen front (dain) is probed on a zeroed throw-away front of its own: the probe then neither counts as a
        front evaluation nor moves the depth net's running statistics."""
        if not hasattr(self.net, 'alloc_front'):
            return {}
        return {'front': self.net.alloc_front(1, frame_shape[1], frame_shape[2], self.device), 'update_stats': False}

    def _shared_fronts(self):
        """Does the plugin have a frozen front that the lockstep / graph paths evaluate once per group and triplet?"""
        return hasattr(self.net, 'front') and bool(getattr(self.net, 'reuse_front', False))

    def _front_passes(self, num_steps, msl, training_phase):
        """One task's forwards in the sequential loop's order, 's' = a support pass (pairs a, b), 't' = a target pass: what
        MetaDAIN.replay_running_stats applies task by task after a group ran its passes with update_stats=False."""
        due = {s for s, _, _ in target_schedule(num_steps, msl, training_phase)}
        passes = ['s'] if self.args.attenuate else []          # L2F: the embedding pass
        for s in range(num_steps + 1):
            passes += ['s'] * (s > 0) + ['t'] * (s in due)      # the step that makes W_s, then the target pass on it
        return passes

    def _routing_known_incomplete(self):
        """True when the routing probe has run and found inner-loop tensors the plugin never reads from the fast dict (graphed
        L2F needs every tensor routed); before the probe has run the answer is 'not known to be incomplete'."""
        return self._routes is not None and bool(self._routes[1])

    def _lockstep_width(self, use_second_order, frame_shape):
        """Tasks per lockstep group, or 0 when this pass must take the sequential loop (second order; L2F on a plugin that
        does not route every tensor: its per-task embedding needs per-task gradients of the plugin's own parameters)."""
        width = int(getattr(self.args, 'task_batch', 0) or 0)
        if width <= 1 or use_second_order:
            return 0
        if not getattr(self.net, 'lockstep_tasks', False):
            # lockstep is OPT-IN per plugin (class attribute `lockstep_tasks = True`): the pass stacks the tasks' samples into
            # one [n*T, ...] batch and hands 5-D stacked weights to MetaConv2dLayer, which is only right for a plugin whose
            # samples never interact (no train-mode BatchNorm) and that reads fast weights through the meta layers only
            return 0
        if hasattr(self.net, 'front') and not self._shared_fronts():
            return 0        # dain with reuse_front = False: the reference's structure, a front per pass, is the sequential loop's
        if not hasattr(self.criterion, 'per_sample'):
            return 0        # a user criterion without per-sample rows: the sequential loop calls it once per task
        if self.args.attenuate and self._routing(frame_shape)[1]:
            return 0
        return width

    def _lockstep_body(self, frames, ids, *, num_steps, msl, training_phase, do_evaluation, importance):
        """What _task_body computes for every task in `ids`, with the T tasks advancing together: activations are
        [n*T, C, H, W] in sample-major order (sample j*T + t belongs to task t), fast weights are stacked [T, *shape], every
        layer is one launch for the whole group (hip_ops.conv_bias_act_tasks), the rule updates the stacked tensors, and the
        criterion is evaluated per sample.  First order only.  Tasks never mix: each task's numbers are those of the
        sequential loop (same kernels per task where the savfi kernels run; MIOpen's grouped solvers elsewhere).

        One difference, invisible in any output: tensors the plugin never reads from the fast dict (SepConv's Subnet /
        Upsample copies) are not carried through step 0.  The reference updates those copies once and never uses them
        (SURVEY.md fact 6); a shared-weight pass cannot give their per-task gradients."""
        T = len(ids)
        routed, _ = self._routing(frames[0].shape[1:])
        theta = self.get_inner_loop_parameter_dict(self.net.named_parameters())
        pick = task_picker(frames, ids)
        W = {k: theta[k].unsqueeze(0).expand(T, *theta[k].shape).contiguous() for k in routed}
        self.inner_loop_optimizer.initialize_state()
        a, b = self.support_idxs
        sup = [torch.cat([pick(a[i]), pick(b[i])], 0) for i in range(3)]           # frame0 | target | frame1, [2T,3,H,W]
        tgt = [pick(i) for i in self.target_idxs]

        # dain: ONE front for the group's [2T] support pairs and one for its [T] target pairs, handed to every pass; the passes leave
        # the depth net's running statistics alone and the updates are replayed below in the sequential loop's order
        sup_kw, tgt_kw = {}, {}
        if self._shared_fronts():
            sup_kw = {'front': self.net.front(sup[0], sup[2]), 'update_stats': False}
            tgt_kw = {'front': self.net.front(tgt[0], tgt[2]), 'update_stats': False}

        def support_loss(weights, num_step):
            # first-order support pass: the plugin's own parameters are constants, weight gradients beside the data-gradient chain
            out = self._run_pass(sup[0], sup[2], weights, num_step, support=True, own_const=True, overlap=self._wgrad_overlap(),
                                 front_kw=sup_kw)
            return self.criterion.per_sample(out, sup[1])['total'].sum()

        due = {s: (index, with_grad) for s, index, with_grad in target_schedule(num_steps, msl, training_phase)}
        task_terms, logs, state = [], [[] for _ in range(T)], {}

        def target(s, weights):
            if s in due:
                index, with_grad = due[s]        # a multi-step-loss pass on W_s is handed num_step = s - 1 (target_schedule)
                with autograd_mode(with_grad):
                    state['preds'] = self._run_pass(tgt[0], tgt[2], weights, s if index is None else s - 1, support=False,
                                                    front_kw=tgt_kw)
                    parts = self.criterion.per_sample(state['preds'], tgt[1])
                task_terms.append(parts['total'] if index is None else importance[index] * parts['total'])
                for k, v in parts.items():
                    for t in range(T):
                        logs[t].append((k, v[t]))

        if self.args.attenuate:        # L2F per task: embedding [T, L] -> gamma [T, L] -> w_i <- gamma_i * w_i
            keys = list(W)
            loss = support_loss(W, 0)
            grads = torch.autograd.grad(loss, [W[k] for k in keys])
            hip_ops.join_weight_gradients()
            emb = hip_ops.mt_mean([g[t] for g in grads for t in range(T)]).view(len(keys), T).t()
            gamma = 1 - self.gamma_mult * self.attenuator(emb)
            gamma.clamp_(0, 1)
            W = {k: gamma[:, i].reshape((T,) + (1,) * (W[k].dim() - 1)) * W[k] for i, k in enumerate(keys)}

        target(0, W)
        for num_step in range(num_steps):
            loss = support_loss(W, num_step)
            keys = list(W)
            grads = torch.autograd.grad(loss, [W[k] for k in keys], allow_unused=True)
            hip_ops.join_weight_gradients()
            W = self.inner_loop_optimizer.update_params(names_weights_dict=W, names_grads_wrt_params_dict=dict(zip(keys, grads)),
                                                        num_step=num_step)
            target(num_step + 1, W)
        if sup_kw:
            self.net.replay_running_stats(sup_kw['front'], tgt_kw['front'], T, self._front_passes(num_steps, msl, training_phase))
        results = self._group_results(frames, ids, torch.stack(task_terms, 0).sum(0), state['preds'], logs, do_evaluation)
        if not training_phase:
            self.net.restore_backup_stats()
        return results

    def _group_results(self, frames, ids, per_task, preds, logs, do_evaluation):
        """The result dicts of a group of tasks from its per-task losses [T], predictions [T,3,H,W] and per task a list of (loss
        part, value); PSNR / SSIM of the T tasks in one call."""
        preds = preds.detach()
        if do_evaluation:
            mse, ssim = self._eval_metrics(preds, frames[self.target_idxs[1]][list(ids)])
            msssim = self._eval_msssim(preds, frames[self.target_idxs[1]][list(ids)])
        results = []
        for t in range(len(ids)):
            res = {'pred': self._to_unit_range(preds[t]).unsqueeze(0), 'logs': logs[t], 'loss': per_task[t]}
            if do_evaluation:
                res['mse'], res['ssim'] = mse[t], ssim[t]
                if msssim is not None:
                    res['msssim'] = msssim[t]
            results.append(res)
        return results

    def _collect(self, num_tasks, local, results, importance, training_phase):
        """Fold the local tasks' results into what forward() returns, (losses, per-task predictions, metrics), and hand what is
        logged to _logging."""
        total_losses, eval_mse, eval_ssim, eval_msssim = [], [], [], []
        deferred = _DeferredMeters()
        preds = [[] for _ in range(num_tasks)]
        for task_id, res in zip(local, results):
            total_losses.append(res['loss'])
            preds[task_id] = res['pred']
            for k, v in res['logs']:
                deferred.add(k, v)
            if 'mse' in res:
                eval_mse.append(res['mse'])
                eval_ssim.append(res['ssim'])
                if 'msssim' in res:
                    eval_msssim.append(res['msssim'])
        # mean over the GLOBAL meta-batch: local sum / B (the all-reduce of grads completes the mean)
        local_sum = torch.sum(torch.stack(total_losses)) if total_losses else torch.zeros((), device=self.device)
        losses = {'loss': local_sum / num_tasks}
        metrics = {'psnr': utils.AverageMeter(), 'ssim': utils.AverageMeter()}
        if getattr(self.args, 'eval_msssim', 0):
            metrics['msssim'] = utils.AverageMeter()
        self._logging(losses, metrics, deferred, eval_mse, eval_ssim, importance, training_phase, eval_msssim)
        return losses, preds, metrics

    def _run_tasks(self, local, body, flatten=None, streams=None):
        """Results of body(task) for the local tasks, in order.  With --task_streams N > 1 on a GPU the tasks are spread
        over N Python threads, each on its own HIP stream: tasks are independent, and the many small kernels of the deep
        layers (a 12x16 map occupies a fraction of the 256 CUs) then overlap with another task's instead of queueing
        behind each other.  Autograd, the caching allocator and MIOpen handles are per-thread / per-stream safe; the
        per-task rule state and the OWN_PARAMS_CONST flag are thread-local."""
        n = min(self._task_streams(graphed=False) if streams is None else streams, len(local))
        if n <= 1 or self.device.type != 'cuda':
            return [body(t) for t in local]
        dev_index = torch.cuda.current_device()
        if self._task_stream_pool is None or len(self._task_stream_pool) < n:
            self._task_stream_pool = [torch.cuda.Stream(device=dev_index) for _ in range(n)]
        streams = self._task_stream_pool[:n]
        cur = torch.cuda.current_stream(dev_index)
        results, errors = {}, []
        flags = (hip_ops.double_backward(), model_utils.fuse_conv_act(), hip_ops.warp_second_order())

        def worker(i):
            try:
                torch.cuda.set_device(dev_index)                # new threads start on device 0
                hip_ops.set_double_backward(flags[0])           # per-thread switches: inherit the caller's
                model_utils.set_fuse_conv_act(flags[1])
                hip_ops.set_warp_second_order(flags[2])
                with torch.cuda.stream(streams[i]):
                    for t in local[i::n]:
                        results[t] = body(t)
            except BaseException as e:                          # re-raised on the calling thread
                errors.append(e)

        for s in streams:
            s.wait_stream(cur)
        threads = [threading.Thread(target=worker, args=(i,), name="savfi-task-%d" % i) for i in range(n)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for s in streams:
            cur.wait_stream(s)
        if errors:
            raise errors[0]
        for packed in results.values():                         # produced on a side stream, consumed on the caller's
            for res in ([packed] if flatten is None else flatten(packed)):
                for v in [res['loss'], res['pred'], res.get('mse'), res.get('ssim'), res.get('msssim')] + [v for _, v in res['logs']]:
                    if torch.is_tensor(v) and v.is_cuda:
                        v.record_stream(cur)
        return [results[t] for t in local]

    def forward(self, data_batch, epoch, use_second_order, use_multi_step_loss_optimization, num_steps,
                training_phase, do_evaluation=False):
        """Outer-loop forward over the (local shard of the) meta-batch  (reference :346-472).
        Returns (losses, per_task_target_preds, metrics)."""
        frames = data_batch
        num_tasks = len(frames[0])
        self._manual_grads = None
        if (graph_inner_loop.supported(self, use_second_order)
                and not (self.args.attenuate and self._routing(frames[0].shape[1:])[1])      # graphed L2F: every tensor routed
                and self._wants_graphs(frames, training_phase)):
            return self._forward_graphed(frames, epoch, use_multi_step_loss_optimization, num_steps, training_phase,
                                         do_evaluation)
        self._set_pass_flags(use_second_order)
        local = self._local_tasks(num_tasks, training_phase)
        msl = bool(use_multi_step_loss_optimization and training_phase
                   and epoch < self.args.multi_step_loss_num_epochs)

        self.net.zero_grad()
        importance = self.get_per_step_loss_importance_vector()

        body = functools.partial(self._task_body, frames, num_steps=num_steps, use_second_order=use_second_order, msl=msl,
                                 training_phase=training_phase, do_evaluation=do_evaluation, importance=importance)
        width = self._lockstep_width(use_second_order, frames[0].shape[1:]) if len(local) > 1 else 0
        if width:
            groups = [local[lo:lo + width] for lo in range(0, len(local), width)]

            def group_body(j):
                group = groups[j]
                if len(group) == 1:
                    return {'group': [body(group[0])]}
                return {'group': self._lockstep_body(frames, group, num_steps=num_steps, msl=msl, training_phase=training_phase,
                                                     do_evaluation=do_evaluation, importance=importance)}
            # --task_streams N > 1: the lockstep groups themselves run concurrently, one thread + HIP stream each
            packed = self._run_tasks(list(range(len(groups))), group_body, flatten=lambda r: r['group'])
            results = [res for p_ in packed for res in p_['group']]
        else:
            results = self._run_tasks(local, body)
        return self._collect(num_tasks, local, results, importance, training_phase)

    def _wants_graphs(self, frames, training_phase):
        """--graph_inner_loop 1: always (where supported); -1 (default): when this rank would otherwise adapt its tasks ONE AT A
        TIME -- a single local task, or a plugin / configuration outside the lockstep path.  A per-task pass is launch-bound
        (CAIN 64x64: 11 steps/s eager, 31 from graphs); a lockstep pass over several tasks is GPU-bound in eager mode already
        and stays there, where every kernel can be timed in place."""
        mode = int(getattr(self.args, 'graph_inner_loop', 0) or 0)
        if mode > 0:
            return True
        local = self._local_tasks(len(frames[0]), training_phase)
        return len(local) <= 1 or self._lockstep_width(False, frames[0].shape[1:]) <= 1

    def _task_streams(self, graphed):
        """--task_streams N: N tasks (or lockstep groups) in flight, one thread + HIP stream each.  -1 (default): one stream for
        the eager loops -- a lockstep pass fills the GPU by itself -- and up to four for hipGraph replays of single tasks, whose
        deep layers occupy a fraction of the 256 CUs (VoxelFlow 256x256, 8 tasks: 137 -> 160 steps/s)."""
        v = int(getattr(self.args, 'task_streams', 1) or 1)
        if v < 0:
            return 4 if graphed else 1
        return max(1, v)

    def _set_pass_flags(self, use_second_order):
        """Per-pass switches of the op layer (thread-local there: task threads inherit them through _run_tasks)."""
        hip_ops.set_double_backward(bool(use_second_order))
        # --warp_second_order 1: the warps' fused twice-differentiable ops (they look at it in second-order passes only)
        hip_ops.set_warp_second_order(bool(int(getattr(self.args, 'warp_second_order', 0) or 0)))
        self._first_order = not use_second_order
        # fused conv epilogues: first-order only (their backward is not differentiable)
        model_utils.set_fuse_conv_act(bool(getattr(self.args, 'fuse_conv_act', 0)) and not use_second_order)

    def _local_tasks(self, num_tasks, training_phase):
        """Training meta-batches are sharded over the ranks (task t -> rank t mod G).  Validation / test sweeps are NOT:
        the data provider hands every rank the full batch (data.py) and ExperimentBuilder consumes every prediction, so each
        rank evaluates all tasks and nothing is reduced -- replicas hold identical weights, hence identical metrics."""
        if not training_phase:
            return list(range(num_tasks))
        return self.task_parallel.local_tasks(num_tasks)

    def _logging(self, losses, metrics, deferred, eval_mse, eval_ssim, importance, training_phase=True, eval_msssim=()):
        """Everything that is logged needs the device to have finished the forward passes.  During training that host sync
        is postponed until the outer backward and the optimizer step are queued (run_train_iter): waiting here would
        drain the queue and the backward would start with the host a whole launch queue behind the GPU."""
        if self._defer_logging:
            importance = importance.detach().clone()      # read later: not the live (learnable) vector an outer step may move
        finish = functools.partial(self._finish_logging, losses, metrics, deferred, eval_mse, eval_ssim, importance,
                                   training_phase, eval_msssim)
        if self._defer_logging:
            self._pending_logging = finish
        else:
            finish()

    def _finish_logging(self, losses, metrics, deferred, eval_mse, eval_ssim, importance, training_phase=True, eval_msssim=()):
        """ONE host sync; fills `losses` and `metrics` in place."""
        meters = deferred.flush()
        if eval_mse:
            mse = torch.stack(eval_mse).cpu().tolist()
            ssims = torch.stack(eval_ssim).cpu()
            for m, s in zip(mse, ssims):
                metrics['psnr'].update(-10 * np.log10(m + 1e-8).item())
                metrics['ssim'].update(s)
        if eval_msssim:
            for v in torch.stack(list(eval_msssim)).cpu().tolist():
                metrics['msssim'].update(v)
        if self.task_parallel.active and training_phase:
            self._reduce_logging(losses, meters, metrics)
        for key, meter in meters.items():
            losses[key] = meter.avg
        weights = importance.detach().cpu().numpy()
        for idx in range(len(weights)):
            losses['loss_importance_vector_{}'.format(idx)] = np.asarray(weights[idx])
        # the device has finished everything these numbers depend on: a bounded wait of the wave-specialised SepConv kernels that
        # gave up (csrc/sepconv_ws.hip) left its count in a mapped host word -- wrong numbers must not be logged as a loss
        _hip.ws_check("meta-iteration at epoch %d" % self.current_epoch)

    def _forward_graphed(self, frames, epoch, use_multi_step_loss_optimization, num_steps, training_phase,
                         do_evaluation):
        """Same contract as forward(), executed by hipGraph replays (graph_inner_loop.py): first-order only, the
        outer gradients are assembled by hand and installed by meta_update()."""
        num_tasks = len(frames[0])
        tp = self.task_parallel
        msl = bool(use_multi_step_loss_optimization and training_phase
                   and epoch < self.args.multi_step_loss_num_epochs)
        self._set_pass_flags(False)
        key = (tuple(frames[0].shape[1:]), num_steps, bool(training_phase), msl)
        local = self._local_tasks(num_tasks, training_phase)
        # --task_batch T: groups of T tasks advance in lockstep through ONE graph set (a shorter last group gets its own);
        # --task_streams N: N graph sets per width (own static buffers and memory pool each), replayed from N threads
        width = max(1, self._lockstep_width(False, frames[0].shape[1:]))
        if self.args.attenuate:
            assert not self._routing(frames[0].shape[1:])[1]
            width = 1          # L2F graph sets hold one task (per-task embedding / gamma between the graphs)
        groups = [local[i:i + width] for i in range(0, len(local), width)]
        n = max(1, min(self._task_streams(graphed=True), len(groups)))

        owner = {tuple(g): j % n for j, g in enumerate(groups)}
        needed = {key + (owner[tuple(g)], len(g)) for g in groups}       # graph sets this call replays: never evicted by it

        def loop_for(i, T):
            k = key + (i, T)
            if k not in self._graphs:
                # a graph set pins its static buffers and memory pool: keep the most recently used ones only (evaluation over
                # clips of many different sizes would otherwise capture, and keep, one set per size) -- but never one this
                # call still needs (more task streams than MAX_GRAPH_SETS / 2 would otherwise evict their own sets)
                cap = max(self.MAX_GRAPH_SETS, len(needed))
                for old in [q for q in self._graphs if q not in needed]:
                    if len(self._graphs) < cap:
                        break
                    self._graphs.pop(old)
                gc.collect()
                self._graphs[k] = graph_inner_loop.GraphedInnerLoop(self, frames[0].shape[1:], num_steps,
                                                                    bool(training_phase), msl, tasks=T)
            else:
                self._graphs[k] = self._graphs.pop(k)          # most recently used last
            return self._graphs[k]
        # capture / look up on THIS thread, before any worker starts: the workers only read the resolved table
        loops = {tuple(g): loop_for(owner[tuple(g)], len(g)) for g in groups}
        importance = self.get_per_step_loss_importance_vector()
        accums = [graph_inner_loop.OuterGradAccumulator(self, self.get_inner_loop_parameter_dict(self.net.named_parameters()))
                  if training_phase else None for _ in range(n)]

        def body(group):
            i = owner[tuple(group)]
            task_losses, preds_g, logs_g = loops[tuple(group)].run_tasks(frames, list(group), importance, accums[i])
            return self._group_results(frames, group, task_losses, preds_g, logs_g, do_evaluation)

        if n == 1:
            grouped = [body(g) for g in groups]
        else:
            index = {j: g for j, g in enumerate(groups)}
            by_index = self._run_tasks(list(index), lambda j: {'group': body(index[j])}, flatten=lambda r: r['group'], streams=n)
            grouped = [r['group'] for r in by_index]
            cur = torch.cuda.current_stream()
            for a in accums:                     # summed on the worker streams, merged / installed on this one
                for t in (a.tensors() if a is not None else []):
                    t.record_stream(cur)
        results = [res for group in grouped for res in group]
        accum = accums[0]
        for other in accums[1:]:
            if other is not None:
                accum.merge(other)
        losses, preds, metrics = self._collect(num_tasks, local, results, importance, training_phase)
        losses['loss'] = losses['loss'].detach()
        if training_phase:
            accum.num_tasks = num_tasks
            self._manual_grads = accum
        return losses, preds, metrics

    def _reduce_logging(self, losses, meters, metrics):
        """Average logging scalars over ranks (second, tiny all-reduce; the loss used for backward stays local)."""
        # fixed key set: a rank whose shard is empty (meta-batch smaller than the world) has no meters of its own
        if hasattr(self.criterion, 'loss_keys'):
            keys = sorted(set(self.criterion.loss_keys()) | set(meters))
        else:                                   # a user criterion: agree on the union of the ranks' keys first
            keys = self.task_parallel.union_of_keys(sorted(meters))
        for k in keys:
            meters.setdefault(k, utils.AverageMeter())
        vec = [float(losses['loss'].detach())]
        for k in keys:
            vec += [float(meters[k].sum), float(meters[k].count)]
        for k in [k for k in ('psnr', 'ssim', 'msssim') if k in metrics]:
            vec += [float(metrics[k].sum), float(metrics[k].count)]
        red = self.task_parallel.allreduce_scalars(torch.tensor(vec, dtype=torch.float64)).cpu().tolist()
        losses['loss_global'] = red[0]
        i = 1
        for k in keys:
            meters[k].sum, meters[k].count = red[i], red[i + 1]
            meters[k].avg = red[i] / max(red[i + 1], 1)
            i += 2
        for k in [k for k in ('psnr', 'ssim', 'msssim') if k in metrics]:
            metrics[k].sum, metrics[k].count = red[i], red[i + 1]
            metrics[k].avg = red[i] / max(red[i + 1], 1)
            i += 2

    # -----------------------------------------------------------------------------------------
    # outer loop entry points (called by ExperimentBuilder)
    # -----------------------------------------------------------------------------------------
    def train_forward_prop(self, data_batch, epoch, do_evaluation=False):
        return self.forward(data_batch=data_batch, epoch=epoch,
                            use_second_order=self.args.second_order and epoch > self.args.first_order_to_second_order_epoch,
                            use_multi_step_loss_optimization=self.args.use_multi_step_loss_optimization,
                            num_steps=self.args.number_of_training_steps_per_iter, training_phase=True,
                            do_evaluation=do_evaluation)

    def evaluation_forward_prop(self, data_batch, epoch):
        return self.forward(data_batch=data_batch, epoch=epoch, use_second_order=False,
                            use_multi_step_loss_optimization=True,
                            num_steps=self.args.number_of_evaluation_steps_per_iter, training_phase=False,
                            do_evaluation=True)

    def _ws_kernels_in_use(self):
        """Does this system's network run the wave-specialised SepConv kernels (the only kernels with bounded in-kernel waits)?"""
        return self.args.model == 'sepconv'

    def meta_update(self, loss):
        """zero_grad -> backward -> (all-reduce of outer grads) -> optimizer step  (reference :551-574)."""
        self.optimizer.zero_grad()
        params = list(self.trainable_parameters())
        # task parallelism: .grad = zeroed views of the flat all-reduce bucket, filled in place by the backward pass
        views = self.task_parallel.prepare_gradients(params)
        if self._manual_grads is not None:        # graphed forward: first-order outer gradients assembled by hand
            reached = self._manual_grads.install(self._manual_grads.num_tasks, into=views)
            if views is not None:
                self.task_parallel.mark_touched(reached)
            self._manual_grads = None
        elif loss.requires_grad:
            loss.backward()
        self.task_parallel.allreduce_gradients(params)
        if self.device.type == 'cuda' and self._ws_kernels_in_use() and _hip.ws_armed():
            # Fail closed: a bounded wait of the wave-specialised SepConv kernels that gave up (csrc/sepconv_ws.hip) has produced wrong
            # gradients.  The stream is drained HERE, before theta moves -- one host wait per meta-iteration, ~0.3 % of a C2 iteration
            # (a figure no kept artefact backs) -- and the exception leaves theta, the optimizer state and the scheduler untouched.
            torch.cuda.current_stream(self.device).synchronize()
            _hip.ws_check("this meta-iteration at epoch %d: its outer step was NOT applied" % self.current_epoch)
        self.optimizer.step()
        if self.device.type == 'cuda':      # the filters every conv layer keeps of its own weight: one launch for all of them
            if self._filter_modules is None:
                self._filter_modules = [m for m in self.net.modules() if isinstance(m, model_utils.MetaConv2dLayer)]
            hip_ops.refresh_module_filters(self._filter_modules)

    def run_train_iter(self, data_batch, epoch, do_evaluation=False):
        _hip.ws_check("an earlier iteration")       # one host word: what a caller that never reads its losses would otherwise miss
        epoch = int(epoch)
        self.current_epoch = epoch
        if not self.training:
            self.train()
        data_batch = [frame.to(device=self.device, non_blocking=True) for frame in data_batch]
        self._defer_logging = True
        try:
            losses, preds, metrics = self.train_forward_prop(data_batch=data_batch, epoch=epoch,
                                                             do_evaluation=do_evaluation)
            self.meta_update(loss=losses['loss'])
            self.optimizer.zero_grad()
            self.zero_grad()
        finally:
            self._defer_logging = False
            finish, self._pending_logging = self._pending_logging, None
        if finish is not None:
            if self.task_parallel.active or not getattr(self.args, 'lazy_logging', 1):
                finish()          # the logging all-reduce is a collective: every rank issues it here, in program order
            else:
                state = {'finish': finish}

                def ensure():
                    f = state.pop('finish', None)
                    if f is not None:
                        f()
                losses, metrics = _LazyLog(losses, ensure), _LazyLog(metrics, ensure)
        return losses, preds, metrics

    def run_validation_iter(self, data_batch):
        _hip.ws_check("an earlier iteration")
        data_batch = [frame.to(device=self.device, non_blocking=True) for frame in data_batch]
        return self.evaluation_forward_prop(data_batch=data_batch, epoch=self.current_epoch)

    def run_test_iter(self, data_batch):
        """Adapt on a 4-frame clip ((0,2)->1, (1,3)->2), then interpolate between frames 1 and 2
        (reference :630-697).  Returns a list of [3,H,W] predictions."""
        _hip.ws_check("an earlier iteration")
        if self.training:
            self.eval()
        frames = [frame.to(device=self.device, non_blocking=True) for frame in data_batch]
        saved = self.support_idxs
        self.support_idxs = [[0, 1, 2], [1, 2, 3]]
        preds = [[] for _ in range(len(frames[0]))]
        self.net.zero_grad()
        # test-time adaptation never back-propagates through the inner loop: first-order passes whatever --second_order says
        # (the reference passes create_graph=args.second_order here, :664, and then discards the graph)
        self._set_pass_flags(False)
        try:
            for task_id in range(len(frames[0])):
                steps = self.args.number_of_evaluation_steps_per_iter
                weights = self._adapt(frames, task_id, steps, False, fronts={} if hasattr(self.net, 'front') else None)
                with torch.no_grad():
                    out, extras = self._run_pass(frames[1][task_id].unsqueeze(0), frames[2][task_id].unsqueeze(0), weights,
                                                 max(steps - 1, 0), support=False, extras=True)
                if extras is not None:         # superslomo (:686-688)
                    out = self.revNormalize(out.squeeze(0)).unsqueeze(0)
                preds[task_id] = out.squeeze(0).detach()
                self.net.restore_backup_stats()
        finally:
            self.support_idxs = saved
        return preds
