"""Rates of the panel's hyper-parameter gradient at the shapes tools/panel_rate.py measures -- B = 4096 series,
M = 128 inducing states 0.25 lengthscales apart, N = 512 points per series, a tenth of them absent:

    matern52-poisson    Matern-5/2 (d = 3), Poisson
    sum5-bernoulli      Sum([Matern32, Matern52]) (d = 5), Bernoulli

Variants, INTERLEAVED (one run of each per repetition after a warm-up of each, in one process), device-event timing, the median and
the spread (min, max) of --reps repetitions, one JSON line per variant:

    model    `update_sites; classic_elbo` (the yardstick: one CVI iteration) and elbo_and_grad on the HIP route
    torch    elbo_and_grad on the torch route of the same object (VIDP_NATIVE_SPARSE_SCORE=0)
    parts    where the HIP route's time goes: the batched Fisher-vector product on the unpacked marginals, the chain score
             (mfgm_packed_kernel_score over the B chains), and mfgm_panel_cond_score (its memset and two launches)

and the peak device memory of one elbo_and_grad per route (torch.cuda.max_memory_allocated).  The kernel's algorithmic bytes are
(2 d + 4) 8 + 4 per point (w, the two gaps, a, b, idx) plus (d + d (d + 1) / 2 + d^2) 8 per inducing state of every series (the packed
marginals, read once), reported as a share of the 8 TB/s peak; the kernel's own time comes from a run of its own,

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/panel_hyper_rate.py --reps 5 --cases parts

    usage: python tools/panel_hyper_rate.py [--reps 30] [--cases model,torch,parts] [--shapes matern52-poisson,sum5-bernoulli]
                                            [--B 4096] [--M 128] [--N 512]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.hyper_rate import HBM_PEAK, emit, interleaved  # noqa: E402
from tools.panel_rate import DZ, kernel, likelihood, make_data  # noqa: E402


def make(name, B, M, N):
    import vidp_amd
    t, y = make_data(name, B, M, N)
    z = torch.arange(M, dtype=torch.float64, device="cuda") * DZ
    m = vidp_amd.PanelSparseCVI(kernel(name), z, likelihood(name), B, learning_rate=0.5)
    data = (torch.from_numpy(t).cuda(), torch.from_numpy(y[..., None]).cuda())
    for _ in range(2):
        m.update_sites(data)
    return m, data


def torch_route(fn):
    os.environ["VIDP_NATIVE_SPARSE_SCORE"] = "0"
    try:
        return fn()
    finally:
        del os.environ["VIDP_NATIVE_SPARSE_SCORE"]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2**20, 1), round(torch.cuda.max_memory_allocated() / 2**20, 1)


def run_shape(name, cases, reps, B, M, N):
    from vidp_amd import FULL, SYM, VEC, hyper, tape
    m, data = make(name, B, M, N)
    k, d = m.kernel, m.kernel.state_dim
    pl = m.dist_p.plan
    assert hyper.panel_native_route(m)
    grad = lambda: m.elbo_and_grad(data)
    runs = {}
    if "model" in cases:
        def step():
            m.update_sites(data)
            return float(m.classic_elbo(data))
        runs["update_sites + classic_elbo"] = step
        runs["elbo_and_grad (HIP route)"] = grad
    if "torch" in cases:
        runs["elbo_and_grad (torch route)"] = lambda: torch_route(grad)
    if "parts" in cases:
        dd, r, s = m._data(data), m._predict_lik(data), m._marginals()["packed"]
        grad()          # leaves the gaps in the data cache
        glo, ghi = dd["gaps"]
        a, b = (r["g1"] + 2.0 * r["g2"] * r["fmu"]).contiguous(), r["g2"].contiguous()
        mu, cov, csub = pl.unpack(VEC, s["x"]), pl.unpack(SYM, s["Sig"]), pl.unpack(FULL, s["Sub"], M - 1)
        _, th_diag, th_sub = m._theta()
        diag, sub = pl.unpack(SYM, th_diag), pl.unpack(FULL, th_sub, M - 1)
        v = [torch.randn_like(mu), torch.randn_like(cov), torch.randn_like(csub)]
        dts = (m.inducing_inputs[1:] - m.inducing_inputs[:-1])[None].expand(B, -1).contiguous()
        kt = k._terms_struct()
        runs["fisher_vector_product"] = lambda: tape.fisher_vector_product(pl, diag, sub, mu, cov, csub, *v)
        runs["chain score (mfgm_packed_kernel_score)"] = lambda: pl.kernel_score(kt, dts, s["x"], s["Sig"], s["Sub"])
        runs["mfgm_panel_cond_score"] = lambda: hyper.conditional_part_panel_native(k, pl, dd, glo, ghi, a, b, s)
    res = interleaved(runs, reps)
    pl.check_info()
    for variant, (ms, all_ms) in res.items():
        extra = {}
        if variant == "mfgm_panel_cond_score":
            nbytes = B * N * ((2 * d + 4) * 8 + 4) + B * M * (d + d * (d + 1) // 2 + d * d) * 8
            extra = dict(algorithmic_bytes=nbytes, share_of_hbm_bound=round(nbytes / HBM_PEAK / (ms * 1e-3), 4))
        emit(shape=name, d=d, B=B, M=M, N=N, variant=variant, ms=round(ms, 4), ms_min=round(min(all_ms), 4), ms_max=round(max(all_ms), 4),
             reps=len(all_ms), **extra)
    hip, tr, st = "elbo_and_grad (HIP route)", "elbo_and_grad (torch route)", "update_sites + classic_elbo"
    if hip in res and st in res:
        emit(shape=name, ratio="elbo_and_grad (HIP route) / (update_sites + classic_elbo)", value=round(res[hip][0] / res[st][0], 3))
    if hip in res and tr in res:
        emit(shape=name, ratio="torch route / HIP route", value=round(res[tr][0] / res[hip][0], 3))
        g, r = hyper.flatten(grad()[1]), hyper.flatten(torch_route(grad)[1])
        emit(shape=name, check="HIP route against the torch route",
             max_rel_diff=max(abs(float(x) - float(y)) / max(1.0, abs(float(y))) for x, y in zip(g, r)))
    if "model" in cases:
        emit(shape=name, peak_memory_mb=dict(zip(("elbo_and_grad (HIP route), above the resident model", "total"), peak_mb(grad))))
    if "torch" in cases:
        emit(shape=name, peak_memory_mb=dict(zip(("elbo_and_grad (torch route), above the resident model", "total"),
                                                 peak_mb(lambda: torch_route(grad)))))
    del m, runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cases", default="model,torch,parts")
    ap.add_argument("--shapes", default="matern52-poisson,sum5-bernoulli")
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--M", type=int, default=128)
    ap.add_argument("--N", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/panel_hyper_rate.py measures on the GPU: no device found")
    for name in args.shapes.split(","):
        run_shape(name, args.cases.split(","), args.reps, args.B, args.M, args.N)


if __name__ == "__main__":
    main()
