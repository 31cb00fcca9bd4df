"""los.LOSChainSummary: the time to turn a field's chains into its map (quantiles of every
parameter, the reddening profile on a grid with its band, mean / std / R-hat, the best sample),
beside the same reduction written with torch ops and beside the host form, in the same run on the
same machine.  Needs a GPU:

    python tools/los_chain_rate.py [--reps 3] [--host-sightlines 8] [--budget-gib 4] [--out FILE]

Workload A: the chains of 1000 sightlines x 32 walkers x 500 kept steps, 4 clouds (N = 16 000
samples per column, 1.5 GB).  Workload B: 10 000 x 32 x 100 (N = 3200, 3.1 GB).  120 grid points,
the five default quantiles.  The chain is on the device, as `LOSFieldSampler.run(device_out=True)`
leaves it.
  (a) device     quantiles, profile, moments + best with `device_out=True`, one synchronisation
  (b) numpy out  the same calls with `device_out=False`
  (c) host form  `LOS_chain_summary_host` on the first `--host-sightlines` sightlines after their
                 copy to the host, copy included, scaled to the field by the number of sightlines
                 (every sightline is computed on its own): an extrapolation
  (d) torch ops  what a user can write without the class, on the device-resident chain: `permute`
                 + `torch.sort` + gather + lerp for the quantiles; the profile evaluated, sorted
                 and reduced in chunks of sightlines under `--budget-gib` of temporaries; mean,
                 std, R-hat and the arg-max with reductions; the same synchronisation
A figure is the median of `--reps` timed runs after a warm-up run, with the spread (min .. max).
The kernel times are HIP events (brutus_enable_timing) of one call each.  Writes
profiles/los_chain_rate.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from brutus_amd import _lib, los  # noqa: E402
from los_rate import kernel_times  # noqa: E402

NCLOUDS, W, NGRID = 4, 32, 120
Q = (.025, .16, .5, .84, .975)


def spread(fn, reps):
    """Seconds of `fn()`: median, min, max over `reps` runs after a warm-up run."""
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return np.median(out[1:]), min(out[1:]), max(out[1:])


def chains(nkept, nsight, seed):
    """(chain, lnl) on the device: thetas spread like a posterior around one profile per sightline,
    the cloud distances ascending."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    P = 4 + 2 * NCLOUDS
    centre = torch.rand((1, nsight, 1, P), generator=g, device="cuda", dtype=torch.float64)
    chain = centre + 0.05 * torch.randn((nkept, nsight, W, P), generator=g, device="cuda", dtype=torch.float64)
    chain[..., :3] = torch.exp(-3. + chain[..., :3])
    chain[..., 4::2] = torch.sort(4. + 15. * chain[..., 4::2], dim=-1).values
    chain[..., 3::2] = torch.sort(3. * chain[..., 3::2].abs(), dim=-1).values
    lnl = -50. + torch.randn((nkept, nsight, W), generator=g, device="cuda", dtype=torch.float64)
    return chain, lnl


def torch_quantiles(cols, q):
    """(..., nq) of cols (..., N): sort, gather, lerp."""
    N = cols.shape[-1]
    xs = torch.sort(cols, dim=-1).values
    pos = q * (N - 1)
    j = pos.floor()
    f = pos - j
    j = j.long()
    x0, x1 = xs[..., j], xs[..., (j + 1).clamp(max=N - 1)]
    return torch.where(f == 0., x0, x0 + f * (x1 - x0))


def torch_summary(chain, lnl, dgrid, q, budget):
    nkept, S, nw, P = chain.shape
    N = nkept * nw
    cols = chain.permute(1, 3, 0, 2)
    quant = torch_quantiles(cols.reshape(S, P, N), q)
    # the profile: per sightline N x ngrid values, their sort (values and indices) and the bins
    per = N * dgrid.numel() * (8 * 3 + 8 + NCLOUDS)
    step = max(1, int(budget // per))
    prof = torch.empty((S, dgrid.numel(), q.numel()), dtype=torch.float64, device=chain.device)
    for a in range(0, S, step):
        th = chain[:, a:a + step].permute(1, 0, 2, 3).reshape(-1, N, P)
        k = (th[:, :, None, 4::2] <= dgrid[None, None, :, None]).sum(dim=-1)
        vals = torch.gather(th, 2, 3 + 2 * k)
        prof[a:a + step] = torch_quantiles(vals.permute(0, 2, 1), q)
    flat = cols.reshape(S, P, N)
    mean, std = flat.mean(dim=-1), flat.std(dim=-1)
    L = nkept // 2
    seqs = torch.cat([cols[..., :L, :], cols[..., nkept - L:, :]], dim=-1)
    Wv = seqs.var(dim=-2).mean(dim=-1)
    BL = seqs.mean(dim=-2).var(dim=-1)
    rhat = torch.sqrt(((L - 1) / L * Wv + BL) / Wv)
    n = torch.nan_to_num(lnl, nan=-float("inf")).permute(1, 0, 2).reshape(S, N).argmax(dim=-1)
    best = chain[n // nw, torch.arange(S, device=chain.device), n % nw]
    return quant, prof, mean, std, rhat, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-sightlines", type=int, default=8)
    ap.add_argument("--budget-gib", type=float, default=4.)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "los_chain_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    dgrid = np.linspace(4., 19., NGRID)
    t_dgrid, t_q = torch.from_numpy(dgrid).cuda(), torch.tensor(Q, dtype=torch.float64, device="cuda")
    lines = ["los.LOSChainSummary, seconds per field (W = %d walkers, %d clouds, %d grid points, %d quantiles)"
             % (W, NCLOUDS, NGRID, len(Q)),
             "(median of %d runs after a warm-up run; min .. max)" % a.reps, torch.cuda.get_device_name(0), ""]
    for label, nsight, nkept in (("A", 1000, 500), ("B", 10000, 100)):
        chain, lnl = chains(nkept, nsight, 7)
        S = los.LOSChainSummary(chain, lnl)

        def device(out):
            return S.quantiles(Q, device_out=out), S.profile(dgrid, Q, device_out=out), S.moments(device_out=out), \
                S.best(device_out=out)
        dev = spread(lambda: device(True), a.reps)
        npy = spread(lambda: device(False), a.reps)
        tor = spread(lambda: torch_summary(chain, lnl, t_dgrid, t_q, a.budget_gib * 2 ** 30), a.reps)
        # the two forms agree (the torch form to rounding: its sums run in another order)
        got, ref = device(True), torch_summary(chain, lnl, t_dgrid, t_q, a.budget_gib * 2 ** 30)
        agree = (float((got[0] - ref[0]).abs().max()), float((got[1] - ref[1]).abs().max()),
                 float((got[2][2] / ref[4] - 1.).abs().max()))
        del ref
        nh = min(a.host_sightlines, nsight)
        t0 = time.perf_counter()
        h = los.LOS_chain_summary_host(chain[:, :nh].cpu().numpy(), lnl[:, :nh].cpu().numpy(), q=Q, dgrid=dgrid)
        host = (time.perf_counter() - t0) * nsight / nh
        same = np.array_equal(h["quantiles"], got[0][:nh].cpu().numpy()) and \
            np.array_equal(h["profile"], got[1][:nh].cpu().numpy())
        L.brutus_enable_timing(1)
        kern = []
        for call in (lambda: S.quantiles(Q, device_out=True), lambda: S.profile(dgrid, Q, device_out=True),
                     lambda: S.best(device_out=True)):
            call()
            kern += kernel_times(L)
        L.brutus_enable_timing(0)
        gb = chain.numel() * 8 / 1e9
        row = ["workload %s: %d sightlines x %d walkers x %d kept steps (N = %d, chain %.2f GB)"
               % (label, nsight, W, nkept, nkept * W, gb),
               "    (a) device, device_out=True     %9.4f s (%.4f .. %.4f) = %.0f sightlines/s" % (dev + (nsight / dev[0],)),
               "    (b) device, numpy out           %9.4f s (%.4f .. %.4f)" % npy,
               "    (c) host form, EXTRAPOLATED from %d sightlines, copy included: %.1f s" % (nh, host),
               "    (d) torch ops, %.0f GiB budget    %9.4f s (%.4f .. %.4f)" % ((a.budget_gib,) + tor),
               "    (d) / (a) = %.2f, (c) / (a) = %.0f" % (tor[0] / dev[0], host / dev[0]),
               "    kernels, ms: " + ", ".join("%s %.3f" % kv for kv in kern),
               "    device = host form to the byte on its %d sightlines (quantiles, profile): %s" % (nh, same),
               "    max |device - torch ops|: quantiles %.3g, profile %.3g; rhat relative %.3g" % agree, ""]
        lines += row
        print("\n".join(row), flush=True)
        del chain, lnl, S, got
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
