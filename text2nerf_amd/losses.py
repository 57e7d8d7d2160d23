"""The two small loss terms the training step of text2nerf_main.py:563-586 applies to the renderer's outputs and
parameters (utils.py:67-80, 488-504), restated so the C3-shaped benchmark step and users of the drop-in have them next to
the renderer. Plain torch ops; the fused forms are optim.TVAdam (TV + Adam) and TensorVMSplit.train_step / t2n_train_loss
(the render loss and its gradients in one kernel)."""
import torch
import torch.nn as nn

from . import _lib


class _TVPlaneSum(torch.autograd.Function):
    """sum_p scale * TVLoss_weight * TVLoss(p) over [1,C,H,W] device planes as two HIP kernels per plane (value: t2n_tv_value,
    gradient: t2n_tv_grad_set) instead of ~15 eager elementwise / reduction kernels per plane with their 69-MB temporaries.
    Same arithmetic as TVLoss.forward (utils.py:488-504) with the sums taken in double."""

    _COEF = {}     # (device, plane shapes) -> [P, 2] normalisers 1 / (c (h-1) w), 1 / (c h (w-1)) as a device tensor (float64)

    @staticmethod
    def forward(ctx, weight, *planes):
        lib = _lib.load()
        dev = planes[0].device
        sums = torch.zeros(len(planes), 32, 2, device=dev, dtype=torch.float64)   # T2N_TV_SLOTS slot pairs per plane
        ctx.weight = float(weight)
        ctx.save_for_backward(*planes)
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for i, p in enumerate(planes):
                b, c, h, w = p.shape
                _lib.check(lib.t2n_tv_value(_lib.ptr(p.detach()), c, h, w, _lib.ptr(sums[i]), st), "t2n_tv_value")
        key = (str(dev), tuple(tuple(p.shape) for p in planes))
        coef = _TVPlaneSum._COEF.get(key)
        if coef is None:
            coef = torch.tensor([[1.0 / (p.shape[1] * (p.shape[2] - 1) * p.shape[3]), 1.0 / (p.shape[1] * p.shape[2] * (p.shape[3] - 1))]
                                 for p in planes], dtype=torch.float64, device=dev)
            _TVPlaneSum._COEF[key] = coef
        # three small device ops for all planes (the host-bound training loop pays ~10 us per eager launch)
        return ((sums.sum(1) * coef).sum() * (2.0 * ctx.weight)).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        planes = ctx.saved_tensors
        dev = planes[0].device
        grads = []
        up = grad_out.detach().to(torch.float32).reshape(1).contiguous()   # the upstream scalar, read on the device by the kernels
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for p in planes:
                b, c, h, w = p.shape
                g = torch.empty_like(p)           # written by the kernel, scaled by the upstream scalar
                _lib.check(lib.t2n_tv_grad_set(_lib.ptr(p.detach()), _lib.ptr(g), c, h, w, ctx.weight, _lib.ptr(up), st), "t2n_tv_grad_set")
                grads.append(g)
        return (None, *grads)


def _is_plain_tvloss(reg):
    """The fused kernels hard-code TVLoss.forward (utils.py:488-504): take them only for that arithmetic — this module's TVLoss,
    the reference's own class (``utils.TVLoss``, matched by qualified name since it cannot be imported here), or a regulariser that
    opts in with ``reg.t2n_fused_tv = True``. A subclass or look-alike with a different forward (L1 TV, masked TV) is called."""
    if getattr(reg, "t2n_fused_tv", False):
        return True
    t = type(reg)
    return t is TVLoss or (t.__name__ == "TVLoss" and t.__module__.split(".")[-1] == "utils")


def tv_planes(reg, planes, scale):
    """sum_p reg(p) * scale for a plain TVLoss `reg` (see _is_plain_tvloss; weight = its float `TVLoss_weight`) on contiguous fp32
    [1,C,H,W] device planes through the HIP kernels; None when that does not apply (the caller then evaluates reg(p) itself)."""
    w = getattr(reg, "TVLoss_weight", None)
    if w is None or not planes or not _is_plain_tvloss(reg):
        return None
    for p in planes:
        if not (p.is_cuda and p.dtype == torch.float32 and p.dim() == 4 and p.shape[0] == 1 and p.shape[2] > 1 and p.shape[3] > 1
                and p.is_contiguous()):
            return None
    return _TVPlaneSum.apply(float(w) * float(scale), *planes)


class _L1Sum(torch.autograd.Function):
    """scale * sum_t mean|t| over contiguous fp32 device tensors (models/tensoRF.py:187-191) as one HIP kernel per tensor each way:
    t2n_l1_value (float64 partial sums, fixed order), t2n_l1_grad_set (scale / numel * sign(t), sign(+-0) = 0, times the device
    upstream scalar)."""

    @staticmethod
    def forward(ctx, scale, *tensors):
        lib = _lib.load()
        dev = tensors[0].device
        sums = torch.empty(len(tensors), _lib.REG_SLOTS, device=dev, dtype=torch.float64)
        ctx.scale = float(scale)
        ctx.save_for_backward(*tensors)
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for i, t in enumerate(tensors):
                _lib.check(lib.t2n_l1_value(_lib.ptr(t.detach()), t.numel(), _lib.ptr(sums[i]), st), "t2n_l1_value")
        return (sums.sum() * ctx.scale).to(torch.float32)      # (the kernel's partial sums are already divided by numel)

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        tensors = ctx.saved_tensors
        dev = tensors[0].device
        up = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        grads = []
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for t in tensors:
                g = torch.empty_like(t)
                _lib.check(lib.t2n_l1_grad_set(_lib.ptr(t.detach()), _lib.ptr(g), t.numel(), ctx.scale, _lib.ptr(up), st), "t2n_l1_grad_set")
                grads.append(g)
        return (None, *grads)


class _OrthoSum(torch.autograd.Function):
    """scale * sum_lines mean_{i != j} |(M M^T)_ij| over line tensors [1,C,n,1] / [C,n,1] (vectorDiffs, models/tensoRF.py:173-182):
    t2n_ortho_value / t2n_ortho_grad_set, the Gram matrix in float64 in a fixed order (see csrc/t2n_reg.hip for why)."""

    @staticmethod
    def forward(ctx, scale, *lines):
        lib = _lib.load()
        dev = lines[0].device
        vals = torch.empty(len(lines), device=dev, dtype=torch.float64)
        ctx.scale = float(scale)
        ctx.save_for_backward(*lines)
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for i, t in enumerate(lines):
                c, n = int(t.shape[-3]), int(t.shape[-2])
                ws = torch.empty(c * c, device=dev, dtype=torch.float64)
                _lib.check(lib.t2n_ortho_value(_lib.ptr(t.detach()), c, n, _lib.ptr(vals[i:]), _lib.ptr(ws), ws.numel() * 8, st),
                           "t2n_ortho_value")
        return (vals.sum() * ctx.scale).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        lines = ctx.saved_tensors
        dev = lines[0].device
        up = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        grads = []
        with torch.cuda.device(dev):
            st = _lib.current_stream_ptr(dev)
            for t in lines:
                c, n = int(t.shape[-3]), int(t.shape[-2])
                g = torch.empty_like(t)
                ws = torch.empty(c * c, device=dev, dtype=torch.float64)
                _lib.check(lib.t2n_ortho_grad_set(_lib.ptr(t.detach()), _lib.ptr(g), c, n, ctx.scale, _lib.ptr(up), _lib.ptr(ws),
                                                  ws.numel() * 8, st), "t2n_ortho_grad_set")
                grads.append(g)
        return (None, *grads)


def _kernel_tensor(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() > 0


def l1_terms(tensors, scale=1.0):
    """scale * sum_t mean|t| (density_L1's sum, models/tensoRF.py:187-191) as a float32 device scalar through the HIP kernels; None
    when they do not apply (CPU, non-float32 or non-contiguous tensors: the caller then evaluates the eager expression)."""
    tensors = list(tensors)
    if not tensors or not all(_kernel_tensor(t) for t in tensors):
        return None
    return _L1Sum.apply(float(scale), *tensors)


def ortho_terms(lines, scale=1.0):
    """scale * sum_lines vectorDiffs(line) (models/tensoRF.py:173-185) for line tensors [1,C,n,1] (or a stacked tensor's [C,n,1]
    slices) as a float32 device scalar through the HIP kernels; None when they do not apply (CPU, non-float32, non-contiguous, or
    C < 2, where the reference takes the mean of an empty tensor)."""
    lines = list(lines)
    if not lines:
        return None
    for t in lines:
        if not (_kernel_tensor(t) and t.dim() in (3, 4) and t.shape[-1] == 1 and (t.dim() == 3 or t.shape[0] == 1) and t.shape[-3] >= 2):
            return None
    return _OrthoSum.apply(float(scale), *lines)


class TVLoss(nn.Module):
    """Total-variation regulariser on a [B,C,H,W] plane (utils.py:488-504)."""

    def __init__(self, TVLoss_weight=1):
        super().__init__()
        self.TVLoss_weight = TVLoss_weight

    def forward(self, x):
        b, c, h, w = x.shape
        dh = x[:, :, 1:, :] - x[:, :, :-1, :]
        dw = x[:, :, :, 1:] - x[:, :, :, :-1]
        return self.TVLoss_weight * 2 * ((dh * dh).sum() / (c * (h - 1) * w) + (dw * dw).sum() / (c * h * (w - 1))) / b


class TransMittanceLoss_mask(nn.Module):
    """MSE of the masked mean weight per ray against 0 (utils.py:67-80)."""

    def __init__(self, device=None):
        super().__init__()

    def forward(self, transmittance, mask):
        mean_trans = torch.mean(transmittance * mask, dim=1)
        return torch.mean(mean_trans ** 2)


# ---- the reference's depth losses (utils.py:301-342) on device tensors: one HIP call each (t2n_depth_loss) ------------------------------
class _DepthLoss(torch.autograd.Function):
    """One of the depth terms of csrc/t2n_depth_loss.hip (kind 1 gnll, 2 si_log, 3 ssi) as (loss, aux): the forward call also writes the
    gradients for upstream gradient 1 (d_depth [R], d_weights [R, N]) and keeps them; the backward multiplies them by grad_output, so
    the function composes with OctreeRender_trilinear_fast(..., is_train=True) in an otherwise unchanged autograd loop. `aux` (4
    float64, on the device) is not differentiable. z_vals gets no gradient (the renderer's sample depths carry none)."""

    @staticmethod
    def forward(ctx, kind, target_std, depth, weights, z_vals, target):
        lib = _lib.load()
        ref = depth if depth is not None else weights
        dev = ref.device
        f32 = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()      # noqa: E731
        dep, w, z, y = f32(depth), f32(weights), f32(z_vals), f32(target)
        R = int(y.shape[0])
        N = int(w.shape[1]) if w is not None else 1
        want_d = depth is not None and ctx.needs_input_grad[2]
        want_w = weights is not None and ctx.needs_input_grad[3] and kind != 2
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        aux = torch.empty(4, device=dev, dtype=torch.float64)
        d_depth = torch.empty(R, device=dev, dtype=torch.float32) if want_d else None
        d_w = torch.empty(R, N, device=dev, dtype=torch.float32) if want_w else None
        ws = torch.empty(int(lib.t2n_depth_loss_workspace_bytes(R)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.t2n_depth_loss(kind, _lib.ptr(dep), _lib.ptr(w), _lib.ptr(z), _lib.ptr(y), R, N, float(target_std), _lib.ptr(loss),
                                          _lib.ptr(aux), _lib.ptr(d_depth), _lib.ptr(d_w), _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream_ptr(dev)), "t2n_depth_loss")
        ctx.grads = (d_depth, d_w)       # this call's own outputs; of the inputs only shape and dtype are needed again
        ctx.like = tuple(None if t is None else (tuple(t.shape), t.dtype) for t in (depth, weights))
        ctx.mark_non_differentiable(aux)
        return loss.reshape(()), aux

    @staticmethod
    def backward(ctx, grad_loss, grad_aux):
        d_depth, d_w = ctx.grads
        depth, weights = ctx.like            # (shape, dtype) of the inputs, or None
        g = grad_loss.detach().to(torch.float32)
        g_depth = g_w = None
        if depth is not None and ctx.needs_input_grad[2]:
            g_depth = (d_depth * g).reshape(depth[0]).to(depth[1])
        if weights is not None and ctx.needs_input_grad[3]:
            g_w = (d_w * g).reshape(weights[0]).to(weights[1]) if d_w is not None \
                else torch.zeros(weights[0], dtype=weights[1], device=g.device)
        return None, None, g_depth, g_w, None, None


def _device_rays(name, **tensors):
    """The shared checks of the depth-loss functions: device tensors (no CPU fallback) of matching ray counts."""
    from ._lib import T2NError
    for k, t in tensors.items():
        if not torch.is_tensor(t):
            raise T2NError(f"{name}: {k} must be a tensor")
        if not t.is_cuda:
            raise T2NError(f"{name}: {k} is on {t.device}; the depth losses run as HIP kernels on device tensors (no CPU fallback)")
    rows = {k: int(t.shape[0]) if t.dim() else -1 for k, t in tensors.items()}
    if len(set(rows.values())) != 1 or -1 in rows.values():
        raise T2NError(f"{name}: the tensors disagree about the number of rays: {rows}")
    return next(iter(rows.values()))


def is_not_in_expected_distribution(depth_mean, depth_var, depth_measurement_mean, depth_measurement_std):
    """utils.py:301-304: the rays a depth measurement does not yet explain — |mean - measurement| exceeds the measurement's standard
    deviation, or the ray's termination variance exceeds the measurement's. Elementwise torch ops; compute_depth_loss evaluates
    the same predicate inside its kernel."""
    off_mean = torch.abs(depth_mean - depth_measurement_mean) - depth_measurement_std
    return (off_mean > 0) | (depth_var > depth_measurement_std * depth_measurement_std)


def compute_depth_loss(depth_map, z_vals, weights, target_depth, target_std=0.1):
    """utils.py:306-320 on device tensors (t2n_depth_loss, kind gnll): the Gaussian negative log-likelihood (nn.GaussianNLLLoss(eps=0.001))
    of the rendered depth under the ray's own termination variance, over the rays is_not_in_expected_distribution selects, as an
    absolute value. Returns the reference's shapes: a scalar, or a (1,) zero tensor that requires grad when no ray is selected or
    there is no ray — which of the two is known on the device only, so this function (like upstream's boolean indexing) waits for
    the kernel; TensorVMSplit.train_step(depth_loss="gnll") does not."""
    if depth_map.shape[0] == 0:
        return torch.zeros((1,), device=depth_map.device, requires_grad=True)
    _device_rays("compute_depth_loss", depth_map=depth_map, z_vals=z_vals, weights=weights, target_depth=target_depth)
    loss, aux = _DepthLoss.apply(1, float(target_std), depth_map, weights, z_vals, target_depth)
    if float(aux[0]) == 0.0:
        return torch.zeros((1,), device=depth_map.device, requires_grad=True)
    return loss


def compute_depth_loss_scale_invariant(depth_map, target_depth):
    """utils.py:324-331 on device tensors (t2n_depth_loss, kind si_log): mean |log depth - log target + alpha| with alpha the mean
    log-ratio. Non-positive depths give NaN / inf, as upstream."""
    _device_rays("compute_depth_loss_scale_invariant", depth_map=depth_map, target_depth=target_depth)
    return _DepthLoss.apply(2, 0.0, depth_map, None, None, target_depth)[0]


def scale_shift_invariant_loss(z_vals, weights, target_depth):
    """utils.py:333-342 on device tensors (t2n_depth_loss, kind ssi): the weighted least-squares fit target ~ s z + t over all samples
    (float64 normal equations on the device instead of statsmodels on a host copy; rank-deficient systems follow the pseudo-inverse),
    then mean(weights (s z + t - target)^2). Returns (loss, s, t). Unlike upstream, `s` and `t` are float64 0-d DEVICE tensors, not
    host floats: nothing is read back. The gradient goes to `weights` alone (the fit sees them detached, as upstream)."""
    _device_rays("scale_shift_invariant_loss", z_vals=z_vals, weights=weights, target_depth=target_depth)
    loss, aux = _DepthLoss.apply(3, 0.0, None, weights, z_vals, target_depth)
    return loss, aux[0], aux[1]


# ---- the distortion regulariser of mip-NeRF 360 on a ray's weights: one HIP call (t2n_distortion_loss) ----------------------------------
class _DistortionLoss(torch.autograd.Function):
    """D of include/t2n.h (t2n_distortion_loss) on the model of _DepthLoss: the forward call also writes d_weights for upstream
    gradient 1 and keeps it; the backward multiplies it by grad_output. z_vals gets no gradient."""

    @staticmethod
    def forward(ctx, inv_range, weights, z_vals):
        lib = _lib.load()
        dev = weights.device
        w, z = (t.detach().to(torch.float32).contiguous() for t in (weights, z_vals))
        R, N = int(w.shape[0]), int(w.shape[1])
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        d_w = torch.empty(R, N, device=dev, dtype=torch.float32) if ctx.needs_input_grad[1] else None
        ws = torch.empty(int(lib.t2n_distortion_loss_workspace_bytes(R)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.t2n_distortion_loss(_lib.ptr(w), _lib.ptr(z), R, N, float(inv_range), _lib.ptr(loss), _lib.ptr(d_w), _lib.ptr(ws),
                                               ws.numel(), _lib.current_stream_ptr(dev)), "t2n_distortion_loss")
        ctx.d_w = d_w
        ctx.like = (tuple(weights.shape), weights.dtype)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        g_w = None
        if ctx.needs_input_grad[1]:
            g_w = (ctx.d_w * grad_loss.detach().to(torch.float32)).reshape(ctx.like[0]).to(ctx.like[1])
        return None, g_w, None


def distortion_loss(weights, z_vals, z_range):
    """The distortion regulariser of mip-NeRF 360 (eq. 15) on device tensors: mean over the rays of sum_ij w_i w_j |m_i - m_j| +
    1/3 sum_i w_i^2 delta_i, with the sample midpoints m and intervals delta of `z_vals` ([R, N], ascending along a ray, as the
    renderer returns them) divided by `z_range` (> 0; near_far[1] - near_far[0] of the field), the last interval 0 — the definition in
    include/t2n.h. Returns a 0-d float32 loss; the gradient goes to `weights` alone. Device tensors only (no CPU fallback). Composes with
    OctreeRender_trilinear_fast(..., is_train=True), which returns weights and z_vals, in an autograd loop;
    TensorVMSplit.train_step(distortion=w) is the form without autograd."""
    from ._lib import T2NError
    _device_rays("distortion_loss", weights=weights, z_vals=z_vals)
    if weights.dim() != 2 or tuple(weights.shape) != tuple(z_vals.shape) or weights.shape[1] == 0:
        raise T2NError(f"distortion_loss: weights {tuple(weights.shape)} and z_vals {tuple(z_vals.shape)} must both be [R, N]")
    z_range = float(z_range)
    if not (z_range > 0.0 and z_range != float("inf")):
        raise T2NError(f"distortion_loss: z_range must be finite and > 0, got {z_range}")
    return _DistortionLoss.apply(1.0 / z_range, weights, z_vals)
