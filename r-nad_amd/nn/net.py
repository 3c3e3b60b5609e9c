"""MLP policy/value net -- drop-in for reference nn/net.py:18-85 (interface + parameter names kept).

The net is two parallel 2-layer perceptrons (10 756 parameters at A = 3, width 256).  north_star kept it in PyTorch-ROCm "unless
rocprof shows the GEMM is large enough to be a dense contraction"; round 1's profile did (the hidden activations of 12.6 M samples
made the torch MLP 99.5 % of a step), so `forward_logits` runs ONE fused fp32-MFMA HIP kernel that keeps the hidden layer in
registers (rnad_mlp_forward), with rnad_mlp_backward as its autograd backward.  The masked exp-normalise policy head (net.py:45-46,
:74-77) and the multinomial sampler (net.py:49) are HIP kernels too.  Shapes the fused kernels do not cover (width not a multiple of
32, non-fp32 weights, a weight image beyond the 160 KiB LDS) and CPU tensors fall back to four torch Linear calls.
`forward_batch` evaluates the net once over the flattened `[T*B, 2A^2]` trajectory -- or, on a tree that is small next to the
batch, over the tree's 2S distinct observations -- instead of a Python loop over t (net.py:67).

State-dict keys (`value_fc0.weight`, ...) are the reference's, so its checkpoints load unchanged.

ConvNet (reference nn/net.py:88-269): the CrossConv tower with a policy and a value head.  With batch_norm=False on the GPU the
whole tower and both heads are ONE fp32-MFMA kernel over a row list (csrc/conv_tower.hip: every CrossConv as two products with
Toeplitz-expanded weights), with rnad_conv_backward as its autograd backward; everything else -- CPU tensors, batch_norm=True,
non-fp32 weights, shapes rnad_conv_supported declines -- runs the plain torch modules.  Observations may be fp16 for either family
(RNaD.obs_half, Episodes(obs_half=True)): an fp16 table holds rounded values, the kernels convert an element as they load it and
compute in fp32, so both families give on an fp16 table what they give on the up-converted one, and no fp32 copy is made.

Both classes expose the same small interface to learn/rnad.py and environment/episode.py (per_row_ready, pack_many, packed_size,
tables_forward, table_forward, backward_rows, ROW_EXTRAS, ROLLOUT_KERNEL; for lazy rows: lazy_rows_ready, LAZY_ROWS_AUTO, staged_actor,
ACTOR_WRITES_VALUE; for the one-launch optimiser tail: optimizer_tail, FUSED_TAIL_AUTO), so the trainer asks the net instead of knowing
its family.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import rnad_hip


class MLP(nn.Module):
    def __init__(self, max_actions, width, device=torch.device("cpu:0"), dtype=torch.float):
        super().__init__()
        self.device = device
        self.value_fc0 = nn.Linear(2 * max_actions**2, width, device=device, dtype=dtype)
        self.value_fc1 = nn.Linear(width, 1, device=device, dtype=dtype)
        self.policy_fc0 = nn.Linear(2 * max_actions**2, width, device=device, dtype=dtype)
        self.policy_fc1 = nn.Linear(width, max_actions, device=device, dtype=dtype)
        self.max_actions = max_actions
        self.width = width
        self._seed = int(torch.randint(0, 2**62, (1,)).item())  # sampler stream of forward(); torch.manual_seed controls it
        self._calls = 0

    # ---------------------------------------------------------------- what RNaD / Episodes ask a net (ConvNet answers the same questions)
    ROW_EXTRAS = True      # the legal fold, row sharding, rnad_mlp_rows_records and rnad_optimizer_step exist for this family
    ROLLOUT_KERNEL = True  # rnad_rollout_run evaluates this net inside the native rollout loop
    LAZY_ROWS_AUTO = True  # RNaD.lazy_rows = None: lazy rows whenever the tree has more rows than the rank plays lanes
    ACTOR_WRITES_VALUE = False  # separate heads: the staged actor is the policy head alone, the value head runs on the visited rows later
    FUSED_TAIL_AUTO = True  # RNaD.fused_optimizer = None: the one-launch optimiser tail whenever it applies

    def optimizer_tail(self, target, exp_avg, exp_avg_sq, steps, hp, images, fold=False):
        """Clip + Adam + EMA of this net (EMA target: `target`, a net of the same shape) in one launch that also keeps `images` = (this
        net's packed image, the target's) current: rnad_optimizer_step.  hp = (lr, beta1, beta2, eps, max_norm, ema)."""
        return rnad_hip.OptimizerStep(self._weights(), exp_avg, exp_avg_sq, steps, target._weights(), *hp, packed=tuple(images),
                                      A=self.max_actions, fold=fold)

    def per_row_ready(self):
        """The fused forward AND backward cover this net: RNaD's per-row step (and its hand-written backward) applies."""
        return self._fusable() and rnad_hip.mlp_backward_supported(self.max_actions, self.width)

    def lazy_rows_ready(self):
        """The family has a staged actor (rnad_mlp_forward_actor): RNaD's lazy-rows step applies."""
        return True

    def staged_actor(self, handle, packed, table, logit, v, policy_rows, fold=False):
        """The closure Episodes.generate(staged_actor=...) calls with row lists: this net's policy head (image `packed`) on those rows of
        the tree's observation `table` -> `logit` and `policy_rows` (v: not written, see ACTOR_WRITES_VALUE).  fold: the FOLD image."""
        fold = handle if fold else False

        def staged_actor(rows, packed=packed, logit=logit, table=table, width=self.width, fold=fold):
            with torch.no_grad():
                rnad_hip.mlp_forward_actor(handle, packed, width, table, logit, policy_rows, rows=rows, fold=fold)

        return staged_actor

    def packed_size(self, fold=False):
        return rnad_hip.mlp_packed_size(self.max_actions, self.width, fold)

    @staticmethod
    def pack_many(nets, out=None, fold=False):
        """The weight images of up to four nets of one shape, in one launch."""
        return rnad_hip.mlp_pack_many([n._weights() for n in nets], nets[0].max_actions, out=out, fold=fold)

    def tables_forward(self, packed_list, table, wants, fold=False, live=None):
        """Nets of this shape (their images) on the same observation table -> [(logits or None, value or None)], in one launch.
        live: a row list -- the other rows are left unwritten (the multi-net launch takes one with the FOLD kernels only)."""
        if live is None:
            return rnad_hip.mlp_forward_multi(packed_list, self.width, table, self.max_actions, wants, fold=fold)
        return rnad_hip.mlp_forward_multi(packed_list, self.width, table, self.max_actions, wants, fold=fold, live=live, zero_rest=False)

    def table_forward(self, packed, table, want_logits=True, want_value=True, live=None, zero_rest=True):
        return rnad_hip.mlp_forward(packed, self.width, table, self.max_actions, want_logits=want_logits, want_value=want_value, live=live,
                                    zero_rest=zero_rest)

    def backward_rows(self, packed, obs, dlogit, dv, live=None, flat=None, views=None, fold=False, capacity=None):
        """dL/dweights for dL/dlogits, dL/dvalue on (the listed rows of) obs, written into `views` -- per-tensor views, in
        _weights() order, of the flat bucket `flat`."""
        return rnad_hip.mlp_backward(packed, self._weights(), obs, self.max_actions, dlogit, dv, live=live, out=views, fold=fold, capacity=capacity)

    # ---------------------------------------------------------------- the two perceptrons
    def _weights(self):
        return [self.value_fc0.weight, self.value_fc0.bias, self.value_fc1.weight, self.value_fc1.bias,
                self.policy_fc0.weight, self.policy_fc0.bias, self.policy_fc1.weight, self.policy_fc1.bias]

    def pack(self):
        """The weight image the fused kernels read (rnad_mlp_pack).  Pack once per net and weight version and hand it to
        every `forward_logits(..., packed=...)` of a rollout; it is NOT cached here (in-place optimizers such as fused
        Adam do not bump tensor versions, so a cache could go stale silently)."""
        if not self._fusable():
            return None
        return rnad_hip.mlp_pack(self._weights(), self.max_actions)

    def _fusable(self):
        """The fused kernels keep ALL weights in the 160 KiB LDS of a CU and tile the hidden layer by 32."""
        w = self.value_fc0.weight
        A, W = self.max_actions, self.width
        image_floats = (2 * A * A + 1) * 2 * W + (1 + A) * W + 12
        return w.is_cuda and w.dtype == torch.float32 and W % 32 == 0 and image_floats * 4 <= 160 * 1024

    def forward_logits(self, input_batch, want_logits=True, want_value=True, packed=None, live=None):
        """obs [N, 2, A, A] (fp32 or fp16) -> logits [N, A], value [N, 1]   (net.py:40-43).

        ONE fused HIP kernel that keeps the hidden layer in registers (rnad_mlp_forward); under autograd it is an
        autograd node whose backward is rnad_mlp_backward (hidden layer recomputed on chip).  Shapes the kernels do not
        cover (width not a multiple of 32, non-fp32 weights, a weight image larger than the LDS) use four PyTorch-ROCm Linear calls.

        live: an rnad_hip.LiveRows over the N samples (ragged trajectories) -- the fused kernels then evaluate those rows only
        and return zeros elsewhere; the PyTorch fallback ignores it and evaluates everything."""
        A = self.max_actions
        if input_batch.is_cuda and self._fusable():
            if not torch.is_grad_enabled():
                return rnad_hip.mlp_forward(packed if packed is not None else self.pack(), self.width, input_batch.contiguous(), A, want_logits,
                                            want_value, live=live)
            if rnad_hip.mlp_backward_supported(A, self.width) and not input_batch.requires_grad:
                packed = packed if packed is not None else self.pack()
                if live is not None:
                    return rnad_hip.FusedMLPRows.apply(input_batch.contiguous(), A, packed, live, *self._weights())
                return rnad_hip.FusedMLP.apply(input_batch.contiguous(), A, packed, *self._weights())
        x = input_batch.reshape(-1, 2 * self.max_actions**2)
        if x.dtype != self.value_fc0.weight.dtype:
            x = x.to(self.value_fc0.weight.dtype)
        value = self.value_fc1(torch.relu(self.value_fc0(x))) if want_value else None
        logits = self.policy_fc1(torch.relu(self.policy_fc0(x))) if want_logits else None
        return logits, value

    @staticmethod
    def _mask(input_batch):
        return input_batch[:, 1, :, 0].to(torch.float).contiguous()  # filter_row (net.py:38)

    # ---------------------------------------------------------------- net.py:37-51
    def forward(self, input_batch):
        logits, value = self.forward_logits(input_batch)
        policy = rnad_hip.policy_head(logits.detach().contiguous(), mask=self._mask(input_batch))
        actions = rnad_hip.sample(policy, seed=self._seed, step=self._calls & 0xFFFFFF, stream_id=2).long()
        self._calls += 1
        return logits, policy, value, actions

    # ---------------------------------------------------------------- net.py:53-62
    def forward_policy(self, input_batch: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            logits, _ = self.forward_logits(input_batch, want_value=False)
        return rnad_hip.policy_head(logits.contiguous(), mask=self._mask(input_batch))

    # ---------------------------------------------------------------- net.py:64-85
    def forward_batch(self, episodes):
        """-> [logit, log_policy, policy, value], shapes [T,B,A] x3 and [T,B,1].  `logit` and `value` carry autograd;
        policy / log_policy come out of the HIP policy head and are constants (the reference's loss never
        differentiates through them: learn/vtrace.py:418, learn/rnad.py:377-382)."""
        T, B = episodes.t_eff + 1, episodes.batch_size
        A = self.max_actions
        logits = value = None
        tree = getattr(episodes, "tree", None)
        if (tree is not None and self._fusable() and rnad_hip.mlp_backward_supported(A, self.width)
                and episodes.indices.dtype == torch.int32 and episodes.indices.is_cuda and B <= 2**21):
            # the observations of a trajectory are rows of the tree's observation table (one per player and state): on a tree that
            # is small next to the batch the net is evaluated on those rows and each slot gathers its own.  Values are the per-slot
            # evaluation's bit for bit; under autograd the weight gradients are summed per row first (rnad_row_sums), i.e. they
            # equal the per-slot ones up to fp32 summation order.  An absorbed slot (index 0) gets the row of state 0, whose
            # observation differs from the zero padding of a collated batch -- those slots are masked by every consumer.
            handle = tree.handle()
            if 8 * handle.S <= T * B:
                table = handle.observations_table(getattr(episodes, "obs_half", False))
                idx = episodes.indices[:T].contiguous()
                if torch.is_grad_enabled():
                    logits, value = rnad_hip.TabularMLP.apply(table, idx, handle, A, self.pack(), *self._weights())
                else:
                    lt, vt = rnad_hip.mlp_forward(self.pack(), self.width, table, A)
                    rows = (idx.long() + (torch.arange(T, device=idx.device) & 1).view(T, 1) * handle.S).reshape(-1)
                    logits, value = lt.index_select(0, rows), vt.index_select(0, rows)
        if logits is None:
            logits, value = self.forward_logits(episodes.observations[:T])
        mask_bits = getattr(episodes, "mask_bits", None)
        if mask_bits is not None:
            policy, log_policy = rnad_hip.policy_head(logits.detach(), mask_bits=mask_bits[:T].reshape(-1), want_log=True)
        else:
            policy, log_policy = rnad_hip.policy_head(logits.detach(), mask=episodes.masks[:T].reshape(-1, A).contiguous(), want_log=True)
        return [logits.view(T, B, A), log_policy.view(T, B, A), policy.view(T, B, A), value.view(T, B, 1)]


# ====================================================================== ConvNet (reference nn/net.py:88-269)
def _factory(device, dtype):
    return {"device": device, "dtype": dtype}


class CrossConv(nn.Module):
    """A filter shaped like a cross: one 1 x (2A-1) kernel along the board rows plus one (2A-1) x 1 kernel along the board columns,
    each over the board zero-padded by A-1 on that axis, so every output cell sees its whole row and its whole column.
    State-dict keys: row_conv.*, col_conv.*."""

    def __init__(self, max_actions, in_channels, out_channels, device=torch.device("cpu:0"), dtype=torch.float):
        super().__init__()
        self.max_actions = max_actions
        taps = 2 * max_actions - 1
        for name, kernel in (("row_conv", (1, taps)), ("col_conv", (taps, 1))):  # registration order = state-dict order
            self.add_module(name, nn.Conv2d(in_channels, out_channels, kernel, **_factory(device, dtype)))

    def forward(self, board):
        reach = self.max_actions - 1
        along_rows = self.row_conv(F.pad(board, (reach, reach)))
        along_cols = self.col_conv(F.pad(board, (0, 0, reach, reach)))
        return along_rows + along_cols


class ConvResBlock(nn.Module):
    """Residual block of two CrossConvs: y = x + norm1(relu(conv1(norm0(relu(conv0(x)))))), the norm AFTER each relu; without
    batch_norm the norms are absent from the state dict.  State-dict keys: conv0.*, conv1.*, batch_norm0.*, batch_norm1.*."""

    def __init__(self, max_actions, channels, batch_norm=False, device=torch.device("cpu:0"), dtype=torch.float):
        super().__init__()
        for name in ("conv0", "conv1"):
            self.add_module(name, CrossConv(max_actions, channels, channels, device, dtype))
        for name in ("batch_norm0", "batch_norm1"):
            self.add_module(name, nn.BatchNorm2d(channels, **_factory(device, dtype)) if batch_norm else nn.Identity())

    def forward(self, x):
        mid = self.batch_norm0(F.relu(self.conv0(x)))
        return x + self.batch_norm1(F.relu(self.conv1(mid)))


class ConvNet(nn.Module):
    """Two-headed CrossConv tower: pre (CrossConv 2 -> channels, no relu), `depth` ConvResBlocks, then a policy and a value Linear on
    the activation flattened in (c, i, j) order.  State-dict keys (pre.*, tower.<d>.*, policy.*, value.*) are the reference's."""

    ROW_EXTRAS = False      # no legal fold, row sharding or fused records launch for this family
    ROLLOUT_KERNEL = False  # the native rollout loop evaluates MLPs only: a ConvNet actor is a table, or is called per step
    LAZY_ROWS_AUTO = False  # lazy rows are opt-in for this family (RNaD.lazy_rows = True): None keeps the all-rows step
    ACTOR_WRITES_VALUE = True  # one tower under both heads: the staged actor launches leave the learner's value on every row they evaluate
    FUSED_TAIL_AUTO = False  # the one-launch optimiser tail is opt-in for this family (RNaD.fused_optimizer = True): None keeps torch's

    def __init__(self, max_actions, channels, depth=1, batch_norm=True, device=torch.device("cpu:0"), dtype=torch.float):
        super().__init__()
        self.device, self.dtype = device, dtype
        self.max_actions, self.channels, self.depth, self.batch_norm = max_actions, channels, depth, bool(batch_norm)
        flat = channels * max_actions * max_actions
        self.pre = CrossConv(max_actions, 2, channels, device, dtype)
        self.tower = nn.ModuleList(ConvResBlock(max_actions, channels, self.batch_norm, device, dtype) for _ in range(depth))
        self.policy = nn.Linear(flat, max_actions, **_factory(device, dtype))
        self.value = nn.Linear(flat, 1, **_factory(device, dtype))
        self._seed = int(torch.randint(0, 2**62, (1,)).item())  # sampler stream of forward(); torch.manual_seed controls it
        self._calls = 0

    # ---------------------------------------------------------------- the fused tower
    def _shape(self):
        return (self.max_actions, self.channels, self.depth)

    def _weights(self):
        """Every parameter in net.parameters() order -- the order of rnad_conv_pack and of the flat gradient bucket."""
        return list(self.parameters())

    def _fusable(self):
        """The tower kernels cover batch_norm=False fp32 nets on the GPU whose shape rnad_conv_supported accepts.  A BatchNorm net
        never takes them (nor any per-row table): in training mode its function depends on the batch it is given."""
        w = self.policy.weight
        return bool(w.is_cuda and w.dtype == torch.float32 and not self.batch_norm and rnad_hip.conv_supported(*self._shape()))

    def pack(self):
        """The packed image of the tower kernels (rnad_conv_pack), or None.  Not cached: see MLP.pack."""
        if not self._fusable():
            return None
        return rnad_hip.conv_pack(self._weights(), *self._shape())

    def per_row_ready(self):
        return self._fusable()

    def lazy_rows_ready(self):
        """The staged actor (rnad_conv_forward_actor) covers this net: RNaD's lazy-rows step applies when asked for."""
        return self._fusable()

    def staged_actor(self, handle, packed, table, logit, v, policy_rows, fold=False):
        """The closure Episodes.generate(staged_actor=...) calls with row lists: tower and both heads (image `packed`) on those rows of
        the tree's observation `table` -> `logit`, `v` and `policy_rows`, one launch per list."""
        assert not fold and v is not None
        shape = self._shape()

        def staged_actor(rows):
            with torch.no_grad():
                rnad_hip.conv_forward_actor(handle, packed, *shape, table, logit, v, policy_rows, rows=rows)

        return staged_actor

    def optimizer_tail(self, target, exp_avg, exp_avg_sq, steps, hp, images, fold=False):
        """MLP.optimizer_tail for this family: rnad_conv_optimizer_step over the 8 + 8 depth tensors, every new weight also written
        into its Toeplitz slots of the two packed images."""
        assert not fold
        return rnad_hip.ConvOptimizerStep(self._shape(), self._weights(), exp_avg, exp_avg_sq, steps, target._weights(), *hp,
                                          packed=tuple(images))

    def packed_size(self, fold=False):
        assert not fold
        return int(rnad_hip.lib().rnad_conv_packed_size(*self._shape()))

    @staticmethod
    def pack_many(nets, out=None, fold=False):
        assert not fold, "the legal fold is an MLP layout"
        outs = [None] * len(nets) if out is None else list(out)
        return [rnad_hip.conv_pack(n._weights(), *n._shape(), out=o) for n, o in zip(nets, outs)]

    def tables_forward(self, packed_list, table, wants, fold=False, live=None):
        """Nets of this shape on the same observation table, a launch each.  live: a row list -- the other rows are left unwritten."""
        assert not fold
        return [rnad_hip.conv_forward(p, *self._shape(), table, want_logits=wl, want_value=wv, live=live, zero_rest=False)
                for p, (wl, wv) in zip(packed_list, wants)]

    def table_forward(self, packed, table, want_logits=True, want_value=True, live=None, zero_rest=True):
        return rnad_hip.conv_forward(packed, *self._shape(), table, want_logits=want_logits, want_value=want_value, live=live,
                                     zero_rest=zero_rest)

    def backward_rows(self, packed, obs, dlogit, dv, live=None, flat=None, views=None, fold=False, capacity=None):
        assert not fold
        return rnad_hip.conv_backward(packed, self._weights(), *self._shape(), obs, dlogit, dv, live=live, out=flat, capacity=capacity)

    def _tower(self, x):
        x = self.pre(x)
        for block in self.tower:
            x = block(x)
        return x.reshape(-1, self.channels * self.max_actions**2)

    def forward_logits(self, input_batch, want_logits=True, want_value=True, packed=None, live=None):
        """obs [N, 2, A, A] -> logits [N, A], value [N, 1]   (net.py:215-221,225).

        Fusable nets on fp32 or fp16 GPU observations: ONE HIP kernel (rnad_conv_forward_obs); under autograd an autograd node whose
        backward is rnad_conv_backward_obs.  live: an rnad_hip.LiveRows over the N samples -- the kernel evaluates those rows only and returns
        zeros elsewhere; the torch fallback ignores it and evaluates everything."""
        A = self.max_actions
        if input_batch.is_cuda and input_batch.dtype in (torch.float32, torch.float16) and self._fusable():
            obs = input_batch.contiguous()
            packed = packed if packed is not None else self.pack()
            if not torch.is_grad_enabled():
                return rnad_hip.conv_forward(packed, *self._shape(), obs, want_logits, want_value, live=live)
            if not input_batch.requires_grad:
                return rnad_hip.FusedConv.apply(obs, self._shape(), packed, live, *self._weights())
        x = input_batch.reshape(-1, 2, A, A)
        if x.dtype != self.policy.weight.dtype:
            x = x.to(self.policy.weight.dtype)
        h = self._tower(x)
        return (self.policy(h) if want_logits else None), (self.value(h) if want_value else None)

    @staticmethod
    def _mask(input_batch):
        return input_batch[:, 1, :, 0].to(torch.float).contiguous()  # filter_row (net.py:214)

    # ---------------------------------------------------------------- net.py:213-227
    # (the reference takes softmax(logits) * mask, renormalised; policy_head takes where(mask, exp(logits), 0), normalised -- the same
    # function up to rounding, and the one its own forward_batch and the MLP use)
    @staticmethod
    def _policy_head(logits, mask):
        """where(mask, exp(logits), 0) / max(sum, 1e-12): rnad_policy_head on the GPU, the same expression in torch on CPU tensors."""
        if logits.is_cuda:
            return rnad_hip.policy_head(logits.contiguous(), mask=mask)
        e = torch.where(mask != 0, torch.exp(logits), torch.zeros_like(logits))
        return e / e.sum(-1, keepdim=True).clamp_min(1e-12)

    def forward(self, input_batch):
        logits, value = self.forward_logits(input_batch)
        policy = self._policy_head(logits.detach(), self._mask(input_batch))
        if policy.is_cuda:
            actions = rnad_hip.sample(policy, seed=self._seed, step=self._calls & 0xFFFFFF, stream_id=2).long()
        else:
            actions = torch.multinomial(policy, num_samples=1).view(-1)
        self._calls += 1
        return logits, policy, value, actions

    # ---------------------------------------------------------------- net.py:229-244
    def forward_policy(self, input_batch: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            logits, _ = self.forward_logits(input_batch, want_value=False)
        return self._policy_head(logits, self._mask(input_batch))

    # ---------------------------------------------------------------- net.py:246-269
    def forward_batch(self, episodes):
        """-> [logit, log_policy, policy, value], shapes [T,B,A] x3 and [T,B,1]; the contract and the table route of MLP.forward_batch
        (the net on the tree's 2S rows when 8 S <= T B, per-slot gradients summed per row before one backward)."""
        T, B = episodes.t_eff + 1, episodes.batch_size
        A = self.max_actions
        logits = value = None
        tree = getattr(episodes, "tree", None)
        if (tree is not None and self._fusable()
                and episodes.indices.dtype == torch.int32 and episodes.indices.is_cuda and B <= 2**21):
            handle = tree.handle()
            if 8 * handle.S <= T * B:
                table = handle.observations_table(getattr(episodes, "obs_half", False))
                idx = episodes.indices[:T].contiguous()
                if torch.is_grad_enabled():
                    logits, value = rnad_hip.TabularConv.apply(table, idx, handle, self._shape(), self.pack(), *self._weights())
                else:
                    lt, vt = rnad_hip.conv_forward(self.pack(), *self._shape(), table)
                    rows = (idx.long() + (torch.arange(T, device=idx.device) & 1).view(T, 1) * handle.S).reshape(-1)
                    logits, value = lt.index_select(0, rows), vt.index_select(0, rows)
        if logits is None:
            logits, value = self.forward_logits(episodes.observations[:T].reshape(-1, 2, A, A))
        mask_bits = getattr(episodes, "mask_bits", None)
        if mask_bits is not None:
            policy, log_policy = rnad_hip.policy_head(logits.detach(), mask_bits=mask_bits[:T].reshape(-1), want_log=True)
        else:
            policy, log_policy = rnad_hip.policy_head(logits.detach(), mask=episodes.masks[:T].reshape(-1, A).contiguous(), want_log=True)
        return [logits.view(T, B, A), log_policy.view(T, B, A), policy.view(T, B, A), value.view(T, B, 1)]
