"""What a render call left in the stream's workspace (carve_workspace, t2n_api.hip: counters | acc | ray_app | app_pos | app_rgb |
app_ray | ...): per-ray records, appearance-list entries and their colours, and the counter block.

`list_shape` asks the library for the list capacity and the offsets it publishes (t2n_render_list_shape); the offsets in between are
rebuilt with carve_workspace's 256-byte rule and checked against the published app_pos offset."""
import ctypes as C

import torch

from text2nerf_amd import _lib, tensorf

K_LISTS = 8
COUNTER_BYTES = K_LISTS * 64 * 4


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def list_shape(R, n, budget=0):
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.load().t2n_render_list_shape(R, n, budget, out), "t2n_render_list_shape")
    return {"list_cap": int(out[0]), "feat_rows": int(out[1]), "fusable": bool(out[2]), "o_pos": int(out[3]), "o_feat": int(out[4]),
            "o_counters": int(out[5])}


def list_capacity(R, n_samples):
    """The worst-case capacity of one sub-list (list_capacity, t2n_api.hip), restated."""
    nblocks = (R + 3) // 4
    return ((nblocks >> 3) + (1 if nblocks & 7 else 0)) * 4 * n_samples + n_samples


def _up(v):
    return (v + 255) // 256 * 256


def offsets(R, n_samples, budget=0):
    s = list_shape(R, n_samples, budget)
    cap = s["list_cap"] * K_LISTS
    o = {"cap": cap, "counters": s["o_counters"]}
    o["acc"] = o["counters"] + _up(COUNTER_BYTES)
    o["ray_app"] = o["acc"] + _up(R * 4)
    o["app_pos"] = o["ray_app"] + _up(R * 16)
    assert o["app_pos"] == s["o_pos"], (o, s)
    o["app_rgb"] = o["app_pos"] + _up(cap * 16)
    o["app_ray"] = o["app_rgb"] + _up(cap * 16)
    return o


def frame_lists(R, n_samples, budget=0, finished=False):
    """The per-ray records and the appearance-list entries the last frame left in the stream's workspace. A ray's slot0 depends on the
    order in which the waves reserved their regions, so the entries are returned ray by ray, in sample order.

    acc [R]; ray_app [R,3] = (n_app, n_valid, first | Lw << 11); slot0 [R] = the raw ray_app.x; entries [total,4] = app_pos,
    app_rgb [total,4] and app_ray [total] of the rays' slices back to back; total. `finished`: rays without a list slice (ray_app.x < 0, coloured by
    k_finish_rays) are allowed and contribute no entries; otherwise such a ray is an error."""
    ws = tensorf._WORKSPACE[tensorf._ws_key(dev())]
    o = offsets(R, n_samples, budget)
    cap = o["cap"]
    acc = ws[o["acc"]:o["acc"] + R * 4].view(torch.float32).clone()
    ray_app = ws[o["ray_app"]:o["ray_app"] + R * 16].view(torch.int32).view(R, 4).clone()
    pos = ws[o["app_pos"]:o["app_pos"] + cap * 16].view(torch.float32).view(cap, 4)
    rgb = ws[o["app_rgb"]:o["app_rgb"] + cap * 16].view(torch.float32).view(cap, 4)
    ray = ws[o["app_ray"]:o["app_ray"] + cap * 4].view(torch.int32)
    n = ray_app[:, 1].long()
    if finished:
        n = torch.where(ray_app[:, 0] >= 0, n, torch.zeros_like(n))
    else:
        assert int(n.min()) >= 0 and int(ray_app[:, 0].min()) >= 0
    start = torch.repeat_interleave(ray_app[:, 0].long(), n)
    first = torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
    idx = start + (torch.arange(int(n.sum()), device=ws.device) - first)
    owner = torch.repeat_interleave(torch.arange(R, device=ws.device), n)
    assert torch.equal(ray[idx].long(), owner)
    return {"acc": acc, "ray_app": ray_app[:, 1:].clone(), "slot0": ray_app[:, 0].clone(), "entries": pos[idx].clone(),
            "app_rgb": rgb[idx].clone(), "app_ray": ray[idx].clone(), "total": int(n.sum())}


def counters_now(R, n, budget=0):
    ws = tensorf._WORKSPACE[tensorf._ws_key(dev())]
    o = list_shape(R, n, budget)["o_counters"]
    return ws[o:o + COUNTER_BYTES].view(torch.int32).clone()
