"""Reading a training step's gradient back out of Adam's moments, in float64.

The fused train step (t2n_train_step) leaves no gradient behind: its Adam consumes and zeroes it. The first moment keeps it, though.
Both Adam kernels (k_adam_multi for the head tensors, adam_one for the channel-last factors, csrc/t2n_optim.hip) update it as
m_t = m_{t-1} + (g - m_{t-1}) * (1 - beta1), so g = m_{t-1} + (m_t - m_{t-1}) / (1 - beta1), with the float32 value of (1 - beta1)
that the kernel multiplies by. Snapshot m_{t-1} before the step (zero before step 1) and the readout is exact to float32 rounding.

Layouts: the 12 factor tensors keep their moments channel-last (optimizer.state[p]["exp_avg_cl"]): a plane [1, C, H, W] as [H, W, C],
a line [1, C, L, 1] as [L, C], both flat. The 7 head tensors keep theirs in the reference layout (state[p]["exp_avg"]).
Everything here is numpy; the field-level readers take a TensorVMSplit and its optim.TVAdam(field=...)."""
import ctypes as C

import numpy as np

F32_BETAS = (float(np.float32(0.9)), float(np.float32(0.99)))      # the betas as the kernels hold them (float arguments)


def one_minus(beta):
    """(1.f - beta) as the kernels evaluate it: both operands float32."""
    return float(np.float32(1.0) - np.float32(beta))


def is_line(i):
    """Kernel order of the 12 factor tensors: density planes 0-2, density lines 3-5, appearance planes 6-8, appearance lines 9-11."""
    return i % 6 >= 3


def cl_to_ref(flat, shape, line):
    """Channel-last flat array -> reference layout `shape` ([1, C, H, W] plane, [1, C, L, 1] line)."""
    flat = np.asarray(flat).reshape(-1)
    if line:
        _, c, n, _ = shape
        return np.ascontiguousarray(flat.reshape(n, c).T[None, :, :, None])
    _, c, h, w = shape
    return np.ascontiguousarray(flat.reshape(h, w, c).transpose(2, 0, 1)[None])


def ref_to_cl(x, line):
    """Reference layout -> channel-last flat array (the inverse of cl_to_ref)."""
    x = np.asarray(x)
    if line:
        return np.ascontiguousarray(x[0, :, :, 0].T).reshape(-1)
    return np.ascontiguousarray(x[0].transpose(1, 2, 0)).reshape(-1)


def recover_grad(m_prev, m_t, one_minus_beta1):
    """The gradient an Adam step consumed, from its first moment before and after (float64)."""
    m_prev = np.asarray(m_prev, np.float64)
    return m_prev + (np.asarray(m_t, np.float64) - m_prev) / float(one_minus_beta1)


def adam_param(p_prev, m_t, v_t, lr, step, beta1, beta2, eps):
    """torch.optim.Adam's parameter update (no weight decay, no amsgrad) from the new moments, in float64:
    p_t = p_{t-1} - lr / (1 - beta1^t) * m_t / (sqrt(v_t) / sqrt(1 - beta2^t) + eps)."""
    bc1 = 1.0 - float(beta1) ** int(step)
    bc2 = 1.0 - float(beta2) ** int(step)
    m_t, v_t = np.asarray(m_t, np.float64), np.asarray(v_t, np.float64)
    return np.asarray(p_prev, np.float64) - (float(lr) / bc1) * m_t / (np.sqrt(v_t) / np.sqrt(bc2) + float(eps))


def adam_second_moment(v_prev, g, beta2, one_minus_beta2):
    """v_t = beta2 v_{t-1} + (1 - beta2) g^2 in float64."""
    g = np.asarray(g, np.float64)
    return float(beta2) * np.asarray(v_prev, np.float64) + float(one_minus_beta2) * g * g


def param_tolerance(p_t, delta, ulps=2.0, rel_update=1e-6):
    """What a float32 Adam update may differ from its float64 recomputation: `ulps` of the new parameter (the final subtraction) plus
    `rel_update` of the update itself (sqrt, the bias-correction factors rounded to float32, a multiply, a divide: ~4.5e-7)."""
    p32 = np.abs(np.asarray(p_t, np.float32))
    return ulps * np.spacing(p32).astype(np.float64) + rel_update * np.abs(np.asarray(delta, np.float64))


# ---- field-level readers ------------------------------------------------------------------------------------------------------------
def kernel_named(f):
    """The 19 tensors in kernel order as (state_dict name, parameter)."""
    name = {id(p): k for k, p in f.named_parameters()}
    return [(name[id(p)], p) for p in f._all_params()]


def snapshot(f, opt):
    """Parameters, first and second moments (reference layout, float64) and the Adam step counts of the 19 tensors. A tensor without
    optimiser state yet has zero moments and step 0. Reads only: nothing about the field or the optimiser changes."""
    out = dict(p={}, m={}, v={}, step={})
    for i, (k, p) in enumerate(kernel_named(f)):
        st = opt.state.get(p, {})
        shape = tuple(p.shape)
        out["p"][k] = p.detach().cpu().numpy().astype(np.float64)
        out["step"][k] = int(st.get("step", 0))
        for key, a, b in (("m", "exp_avg_cl", "exp_avg"), ("v", "exp_avg_sq_cl", "exp_avg_sq")):
            if i < 12 and a in st:
                out[key][k] = cl_to_ref(st[a].detach().cpu().numpy().astype(np.float64), shape, is_line(i))
            elif i >= 12 and b in st:
                out[key][k] = st[b].detach().cpu().numpy().astype(np.float64).reshape(shape)
            else:
                out[key][k] = np.zeros(shape, np.float64)
    return out


def shard_offsets(f):
    """(offset, floats) of each factor tensor in the field's flat channel-last gradient buffer (256-B aligned slices)."""
    from text2nerf_amd import _lib
    lay = (C.c_int64 * 36)()
    _lib.check(_lib.load().t2n_field_shard_layout(f._handle, 1, lay), "t2n_field_shard_layout")
    return [(int(lay[3 * t]), int(lay[3 * t + 2])) for t in range(12)]


def factor_grads_ref(f):
    """The field's factor gradient buffer (as it stands) in the reference layout, float64, by state_dict name."""
    buf = f.factor_grad_buffer(_raw=True).detach().cpu().numpy()
    out = {}
    for i, ((k, p), (off, n)) in enumerate(zip(kernel_named(f)[:12], shard_offsets(f))):
        assert n == p.numel(), (k, n, p.numel())
        out[k] = cl_to_ref(buf[off:off + n].astype(np.float64), tuple(p.shape), is_line(i))
    return out


def master_copies(f):
    """The 12 channel-last float32 master copies the kernels read (t2n_field_factor_buffer), in the reference layout, by name."""
    import torch
    from text2nerf_amd import _lib
    from text2nerf_amd.parallel import _DeviceView
    lib = _lib.load()
    dev = f.basis_mat.weight.device
    out = {}
    for i, (k, p) in enumerate(kernel_named(f)[:12]):
        ptr = C.c_void_p()
        _lib.check(lib.t2n_field_factor_buffer(f._handle, i, C.byref(ptr)), "t2n_field_factor_buffer")
        flat = torch.as_tensor(_DeviceView(ptr.value, p.numel()), device=dev).cpu().numpy()
        out[k] = cl_to_ref(flat, tuple(p.shape), is_line(i))
    return out


def train_record(f):
    """t2n_field_train_record: [0] sequence, [1] Adam steps applied, [2] steps withheld, then the per-step records."""
    from text2nerf_amd import _lib
    rec = (C.c_uint32 * 36)()
    _lib.check(_lib.load().t2n_field_train_record(f._handle, rec), "t2n_field_train_record")
    return list(rec)
