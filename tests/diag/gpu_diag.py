#!/usr/bin/env python3
"""Stage-by-stage comparison of the HIP path against oracle #2 (fp64) on the GPU box.
Prints max-abs / relative error of every intermediate; never stops at the first mismatch.
usage: python tools/gpu_diag.py [subset|full] [tier_wave tier_block]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from mllp_amd import _lib  # noqa: E402
from mllp_amd.data import SUBSET5, load_packed  # noqa: E402
from mllp_amd.graph import LPBatch, adam_step  # noqa: E402
from oracle import pyg_restatement as o1  # noqa: E402
from oracle import spmm_form as o2  # noqa: E402


def err(name, got, want, tol=1e-5, atol=0.0):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        print(f"  {name:28s} SHAPE {got.shape} vs {want.shape}")
        return False
    d = np.abs(got - want)
    scale = max(np.abs(want).max(), 1e-30) if want.size else 1.0
    bad = not np.isfinite(got).all()
    rel = d.max() / scale if want.size else 0.0
    flag = "OK " if ((rel < tol or (want.size and d.max() <= atol)) and not bad) else "BAD"
    where = int(np.argmax(d)) if want.size else -1
    print(f"  {flag} {name:28s} maxabs={d.max() if want.size else 0:.3e} rel_to_max={rel:.3e} scale={scale:.3e} argmax={where}"
          + (" NONFINITE" if bad else ""))
    return flag == "OK "


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "subset"
    tw = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    tb = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    inst = load_packed(SUBSET5) if which == "subset" else load_packed()
    print(f"== {which}: {len(inst)} instances, tiers=({tw},{tb}) device={torch.cuda.get_device_name(0)}")
    t0 = time.time()
    batch = LPBatch.from_instances(inst, tier_wave=tw, tier_block=tb)
    print("graph dims", batch.dims(), f"build {time.time()-t0:.2f}s")
    ob = o2.BatchCSR(inst)
    ok = True
    # graph arrays
    ok &= err("csr_ptr", batch.export(0), ob.rp)
    ok &= err("csr_idx", batch.export(1), ob.ci)
    ok &= err("csr_val", batch.export(2), ob.va.astype(np.float32))
    ok &= err("csc_ptr", batch.export(3), ob.cp)
    ok &= err("csc_idx", batch.export(4), ob.ri)
    ok &= err("csc_val", batch.export(5), ob.cv.astype(np.float32))
    # spmm
    rng = np.random.default_rng(0)
    Hn = rng.standard_normal((batch.N, 16)).astype(np.float32)
    Hm = rng.standard_normal((batch.M, 16)).astype(np.float32)
    Y = batch.spmm(torch.tensor(Hn, device="cuda")).cpu().numpy()
    ok &= err("spmm A@H", Y, o2.spmm(ob.rp, ob.ci, ob.va.astype(np.float32).astype(np.float64), Hn.astype(np.float64)))
    Yt = batch.spmm(torch.tensor(Hm, device="cuda"), transpose=True).cpu().numpy()
    ok &= err("spmm At@H", Yt, o2.spmm(ob.cp, ob.ri, ob.cv.astype(np.float32).astype(np.float64), Hm.astype(np.float64)))

    sd = o1.init_state(42, torch.float64)
    sd_np = {k: v.numpy() for k, v in sd.items()}
    flat32 = o1.flatten_state(sd).float().cuda()
    # single layers
    for name, dst_is_var, cin in (("gconv1_w2s", True, 1), ("gconv1_s2w", False, 1), ("gconv2_w2s", True, 16),
                                  ("gconv2_s2w", False, 16)):
        p = o2.conv_params(sd_np, name)
        ptr, idx, val, nd, ns = ob.orient(dst_is_var)
        xs = (rng.standard_normal((ns, cin)) * 0.7).astype(np.float32).astype(np.float64)
        xd = (rng.standard_normal((nd, cin)) * 0.7).astype(np.float32).astype(np.float64)
        h_ref, saved = o2.conv_fwd(p, ptr, idx, val, xs, xd)
        cp = flat32[_lib.conv_param_slice(name)].contiguous()
        ws = batch.tconv_workspace(dst_is_var, cin)
        xs_t = torch.tensor(xs, dtype=torch.float32, device="cuda").contiguous()
        xd_t = torch.tensor(xd, dtype=torch.float32, device="cuda").contiguous()
        h = batch.tconv_fwd(dst_is_var, cin, cp, xs_t, xd_t, ws)
        torch.cuda.synchronize()
        print(f" layer {name} (dst_is_var={dst_is_var}, cin={cin})")
        ok &= err("h", h.cpu().numpy(), h_ref)
        # saved intermediates (layout of ConvWs in api.cpp::conv_ws_carve)
        up16 = lambda x: (x + 15) // 16 * 16
        o_ = up16(1088)
        wsn = ws.cpu().numpy()
        qp = wsn[o_:o_ + nd * cin].reshape(nd, cin); o_ += up16(nd * cin)
        t = wsn[o_:o_ + nd]; o_ += up16(nd)
        Z = wsn[o_:o_ + nd * cin].reshape(nd, cin); o_ += up16(nd * cin)
        aux = wsn[o_:o_ + nd * 4].reshape(nd, 4); o_ += up16(nd * 4)
        if cin == 16:
            ok &= err("qp", qp, saved["qp"])
            ok &= err("t", t, saved["t"])
        ok &= err("Z", Z, saved["Z"])
        ok &= err("aux.u", aux[:, 0], saved["u"])
        ok &= err("aux.mx", aux[:, 1], saved["mx"], tol=1e-4)
        ok &= err("aux.rinv", aux[:, 2], saved["rinv"])
        ok &= err("aux.S", aux[:, 3], saved["S"])
        dh = rng.standard_normal((nd, 16)).astype(np.float32).astype(np.float64)
        grads, dxd, dxs, inter = o2.conv_bwd(p, ptr, idx, val, xs, xd, saved, dh, need_input_grads=(cin == 16))
        pg, dxd_g, dxs_g, g_masked = batch.tconv_bwd(dst_is_var, cin, cp, xs_t, xd_t, h, ws,
                                                     torch.tensor(dh, dtype=torch.float32, device="cuda"))
        torch.cuda.synchronize()
        ok &= err("g (masked dh)", g_masked.cpu().numpy(), inter["g"])
        wsn = ws.cpu().numpy()
        recw = 40 if cin == 16 else 8
        rec = wsn[o_:o_ + nd * recw].reshape(nd, recw); o_ += up16(nd * recw)
        dqp = wsn[o_:o_ + nd * cin].reshape(nd, cin); o_ += up16(nd * cin)
        dsdt = wsn[o_:o_ + nd * 2].reshape(nd, 2); o_ += up16(nd * 2)
        if cin == 16:
            ok &= err("rec.gv", rec[:, 16:32], inter["gv"])
            ok &= err("rec.ge", rec[:, 35], inter["ge"])
            ok &= err("rec.c", rec[:, 36], inter["c"], tol=1e-4)
        else:
            ok &= err("rec.gv", rec[:, 1], inter["gv"][:, 0])
            ok &= err("rec.c", rec[:, 6], inter["c"], tol=1e-4)
        ok &= err("dqp", dqp, inter["dqp"], tol=3e-5)
        ok &= err("ds", dsdt[:, 0], inter["ds"], atol=1e-5)    # ~0 by construction (softmax shift invariance)
        ok &= err("dt", dsdt[:, 1], inter["dt"], tol=3e-5)
        if cin == 16:
            ok &= err("dx_dst", dxd_g.cpu().numpy(), dxd, tol=3e-5)
            ok &= err("dx_src", dxs_g.cpu().numpy(), dxs, tol=3e-5)
        pgn, o3 = pg.cpu().numpy(), 0
        for key in ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight",
                    "lin_value.bias", "lin_edge.weight", "lin_skip.weight", "lin_skip.bias"):
            ref = np.asarray(grads[key]).reshape(-1)
            ok &= err("grad " + key, pgn[o3:o3 + ref.size], ref, tol=5e-5, atol=1e-6 if key == "lin_key.bias" else 0.0)
            o3 += ref.size

    # whole model
    print(" whole model")
    r = o2.gnn_forward_backward(sd_np, ob)
    logits = batch.forward(flat32)
    torch.cuda.synchronize()
    ok &= err("logits (forward)", logits.cpu().numpy(), r["logits"])
    wsn = None
    loss, logits2, grads = batch.loss_step(flat32)
    torch.cuda.synchronize()
    ok &= err("logits (loss_step)", logits2.cpu().numpy(), r["logits"])
    ok &= err("loss", loss.cpu().numpy(), np.array([r["loss"]]))
    gn, off = grads.cpu().numpy(), 0
    allok = err("grads (all)", gn, r["grads"], tol=5e-5)  # lin_key.bias grads are ~0 (noise) on both sides
    ok &= allok
    if not allok:
        for k, s in o1.state_dict_spec():
            c = int(np.prod(s))
            err("  " + k, gn[off:off + c], r["grads"][off:off + c], tol=5e-5)
            off += c
    # backward from dlogits (drop-in path)
    dz = ob.wnode * (1.0 / (1.0 + np.exp(-r["logits"])) - ob.basis)
    g2 = batch.backward(flat32, torch.tensor(dz, dtype=torch.float32, device="cuda"))
    ok &= err("grads (fwd + bwd API)", g2.cpu().numpy(), r["grads"], tol=5e-5)
    # adam
    p = flat32.clone()
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    state = torch.tensor([0.0, 1e-3, 0.9, 0.999], device="cuda")
    pr = o1.flatten_state(sd).numpy().copy(); mr = np.zeros_like(pr); vr = np.zeros_like(pr)
    for step in (1, 2, 3):
        adam_step(p, grads, m, v, state)
        o2.adam_step(pr, r["grads"], mr, vr, step)
    torch.cuda.synchronize()
    # lin_key.bias is a dead parameter (a per-destination constant cancels in softmax): its gradient is
    # rounding noise on both sides and Adam normalises noise to O(lr) moves -> excluded from the comparison
    keep = np.ones(pr.size, bool)
    off = 0
    for k, s in o1.state_dict_spec():
        c = int(np.prod(s))
        if k.endswith("lin_key.bias"):
            keep[off:off + c] = False
        off += c
    ok &= err("adam x3 params", p.cpu().numpy()[keep], pr[keep], tol=1e-5)
    ok &= err("adam state.step", state.cpu().numpy()[:1], np.array([3.0]))
    # metrics
    met = batch.topm_metrics(logits).cpu().numpy()
    ref = np.array([o1.topk_metrics(z, i.m, i.basis) for z, i in
                    zip(batch.logits_per_instance(logits.cpu().numpy()), inst)])
    ok &= err("metrics correct", met[:, 0], ref[:, 0], tol=1e-6)
    ok &= err("metrics f1", met[:, 1], ref[:, 1], tol=1e-5)
    print("ALL OK" if ok else "SOME STAGES BAD")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
