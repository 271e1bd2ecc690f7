#!/usr/bin/env python3
"""Times of the HGCal geometry decode on the GPU, at HGCal's shape (28 layers, 252 bins, 3000 cells):

    python tools/geom_bench.py [--batch 16 --seconds 1.0 --out geom_bench.json]

  dec            cd_geom_apply on the packed map           against   torch.einsum over the dense (L, N, E) matrix
  sparse         cd_geom_decode_sparse (Philox uniforms)   against   generate_sparse_mat's operations in torch on the device
                                                                     (a (B, L, N, E) matrix per call) + its einsum
  --case model   HGCal's in-model embedding (cd_plan_set_geom) at the real shape -- (28, 12, 21) grid, 1988 cells, batch 16 --
                 against the pre-embedded `hgcal` config on the same U-Net: denoise and the training step (loss + backward) with
                 frozen and with trainable maps, and FusedAdam's step with and without the two dense map parameters.  The masks
                 have init_map's sparsity (a cell's own bins plus its neighbourhood, about five entries a cell).
The torch forms are the comparison, not code under test.  The map is synthetic (one or two non-zeros per cell, seeded).  Each
timing is a loop of back-to-back calls for --seconds between two device events, after a warm-up; the shader clock is sampled
meanwhile (tools/clock_trace.py's sampler).  Outputs of the two forms are compared before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def synthetic_maps(L, E, N, seed=7):
    rng = np.random.default_rng(seed)
    enc = np.zeros((L, E, N), dtype=np.float32)
    ll, nn = np.meshgrid(np.arange(L), np.arange(N), indexing="ij")
    e1 = rng.integers(0, E, size=(L, N))
    two = rng.random((L, N)) < 0.3
    e2 = (e1 + 1 + rng.integers(0, E - 1, size=(L, N))) % E
    enc[ll, e1, nn] = np.where(two, 0.5, 1.0)
    enc[ll[two], e2[two], nn[two]] = 0.5
    dec = np.ascontiguousarray(enc.transpose(0, 2, 1))
    return enc, (dec / np.maximum(dec.sum(1, keepdims=True), 1e-30)).astype(np.float32)


def torch_sparse_decode(mat, z, eps=1e-6):
    """The operations of generate_sparse_mat (per shower) and the decoder's einsum, on the device."""
    m = mat.repeat((z.shape[0], 1, 1, 1))
    mask = m > eps
    r = torch.rand_like(m) * mask + m
    r = r.scatter(-2, torch.argmax(r, dim=-2, keepdim=True), 1.0 + eps)
    s = (r > 1.0).to(torch.float32)
    s /= torch.sum(s, dim=-2, keepdim=True)
    s *= mask
    return torch.einsum("b l n e, b c l e -> b c l n", s, z)


def timed(forms, seconds, result, smp, phase_summary):
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        smp.phase = name
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n, t0 = 0, time.perf_counter()
        e0.record()
        while time.perf_counter() - t0 < seconds:
            for _ in range(10):
                fn()
            n += 10
            torch.cuda.synchronize()
        e1.record()
        torch.cuda.synchronize()
        smp.phase = "idle"
        result[name] = dict(calls=n, us_per_call=round(e0.elapsed_time(e1) * 1e3 / n, 2), **phase_summary(smp, name))
        print(name, json.dumps(result[name]), flush=True)


def model_case(a, smp, phase_summary):
    """the in-model embedding against the pre-embedded config: what the added launches cost per denoise and per training step"""
    from calodiffusion_amd import hgcal
    from calodiffusion_amd.calodiffusion import CaloDiffusion
    from calodiffusion_amd.configs import load_config
    from calodiffusion_amd.optim import FusedAdam
    L, A, R, N, B = 28, 12, 21, 1988, a.batch
    E = A * R
    enc_mat, dec_mat = synthetic_maps(L, E, N)
    rng = np.random.default_rng(11)
    enc_mask = enc_mat != 0
    ll, nn = np.meshgrid(np.arange(L), np.arange(N), indexing="ij")
    for _ in range(4):  # the neighbourhood of a cell's bin
        enc_mask[ll, rng.integers(0, E, size=(L, N)), nn] = True
    dec_mask = dec_mat != 0
    base = dict(load_config("hgcal"))
    cell = dict(base, SHOWER_EMBED="NN", SHAPE_PAD=[-1, 1, L, N])
    models = {}
    for name, cfg in (("pre_embed", base),
                      ("frozen", dict(cell, NN_EMBED=hgcal.HGCalConverter.from_matrices([L, A, R], enc_mat, dec_mat))),
                      ("trainable", dict(cell, TRAINABLE_EMBED=True, NN_EMBED=hgcal.HGCalConverter.from_matrices(
                          [L, A, R], enc_mat, dec_mat, enc_mask, dec_mask, trainable=True)))):
        torch.manual_seed(1234)
        models[name] = CaloDiffusion(cfg, n_steps=cfg["NSTEPS"], loss_type="l2")
    gen = torch.Generator().manual_seed(1)
    Ein, layers = torch.rand((B, 3), generator=gen).cuda(), torch.randn((B, L + 1), generator=gen).cuda()
    sigma = (torch.randn((B,), generator=gen) * 1.2 - 1.2).exp().cuda()
    state = {k: torch.randn((B,) + tuple(m._data_shape), generator=gen).cuda() for k, m in models.items()}
    noise = {k: torch.randn(v.shape, generator=gen).cuda() for k, v in state.items()}
    opts = {k: FusedAdam(m.parameters(), lr=1e-4) for k, m in models.items() if k != "frozen"}

    def denoise(k):
        with torch.no_grad():
            return models[k].denoise(state[k], E=Ein, sigma=sigma, layers=layers)

    def step(k):
        models[k].zero_grad()
        models[k].compute_loss(state[k], Ein, noise=noise[k], layers=layers).backward()

    forms = {}
    for k in models:
        forms[f"denoise_{k}"] = lambda k=k: denoise(k)
        forms[f"train_step_{k}"] = lambda k=k: step(k)
    for k in opts:
        step(k)
        forms[f"adam_{k}"] = lambda k=k: opts[k].step()
    result = {"shape": {"L": L, "E": E, "N": N, "B": B}, "enc_masked": int(enc_mask.sum()), "dec_masked": int(dec_mask.sum()),
              "dense_slot_floats": 2 * L * E * N}
    timed(forms, a.seconds, result, smp, phase_summary)
    for what in ("denoise", "train_step"):
        for k in ("frozen", "trainable"):
            result[f"{what}_{k}_extra_us"] = round(result[f"{what}_{k}"]["us_per_call"] - result[f"{what}_pre_embed"]["us_per_call"], 2)
    result["adam_dense_maps_extra_us"] = round(result["adam_trainable"]["us_per_call"] - result["adam_pre_embed"]["us_per_call"], 2)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default="geom_bench.json")
    ap.add_argument("--case", default="decode", choices=("decode", "model"))
    a = ap.parse_args()
    from calodiffusion_amd import hgcal
    from clock_trace import Sampler, phase_summary
    if a.case == "model":
        smp = Sampler(5e-3)
        smp.th.start()
        result = model_case(a, smp, phase_summary)
        smp.stop = True
        smp.th.join()
        result["clock_source"] = smp.source
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        json.dump(result, open(a.out, "w"), indent=1)
        print(json.dumps(result))
        return
    L, A, R, N, B = 28, 12, 21, 3000, a.batch
    enc_mat, dec_mat = synthetic_maps(L, A * R, N)
    conv = hgcal.HGCalConverter.from_matrices([L, A, R], enc_mat, dec_mat)
    dense = torch.from_numpy(dec_mat).cuda()
    z = torch.rand((B, 1, L, A, R), generator=torch.Generator().manual_seed(1)).cuda()
    zf = z.reshape(B, 1, L, A * R)
    forms = {
        "dec_packed": lambda: conv.dec(z),
        "dec_einsum": lambda: torch.einsum("l n e, ... l e -> ... l n", dense, zf),
        "sparse_packed": lambda: conv.dec(z, sparse_decoding=True, seed=5, offset=0),
        "sparse_torch": lambda: torch_sparse_decode(dense, zf),
    }
    ref, got = forms["dec_einsum"](), forms["dec_packed"]()
    check = {"dec_max_abs_diff": float((ref - got).abs().max()), "dec_max_abs": float(ref.abs().max())}
    sp = forms["sparse_packed"]()
    check["sparse_layer_sum_rel_diff"] = float(((sp.sum(-1) - forms["sparse_torch"]().sum(-1)).abs() / sp.sum(-1).abs().clamp_min(1e-30)).max())
    print(json.dumps(check))
    smp = Sampler(5e-3)
    smp.th.start()
    result = {"shape": {"L": L, "E": A * R, "N": N, "B": B}, "check": check,
              "nnz": int((dec_mat != 0).sum()), "dense_bytes": dec_mat.nbytes}
    timed(forms, a.seconds, result, smp, phase_summary)
    smp.stop = True
    smp.th.join()
    result["clock_source"] = smp.source
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
