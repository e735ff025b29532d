"""Cost of joint segmentations on the C2 workload (tools/bench_sg.py: 28M CpG
over 22 chromosomes, 4 samples, K = 6, N_max = 250): the untraced forward-only
launch, the history launch (hyg_sg_history_chains_multi), the sampler alone
(hyg_sg_sample_paths_multi, B = 25), history bytes and the sampler's share.

    python tools/bench_sg_sample.py [--sites N] [--repeats R] [--history-gib G] [--out FILE]

Two parts. "chr1": the longest chain alone; the forward-only and the history
launch alternate R times, so that their difference stands against the spread
of either. "genome": the 22 chains; the forward-only launch holds all of them
at once, the history launches run in the groups of `hygeia sg_sample_genome`
(single_group.history_groups under --history-gib), each followed by its
sampler launch, the history buffer reused. Times are device events around each
launch on one stream. The untraced launch is the multi-model forward-only
build with one model, the build the history build is derived from; this
change leaves its code as it was (profiles/sg_sample_resource_notes.txt), so
its time is the parent commit's. Prints one JSON object.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    xs = [float(x) for x in xs]
    return {"runs_ms": xs, "median_ms": float(np.median(xs)), "min_ms": min(xs), "max_ms": max(xs),
            "spread_ms": max(xs) - min(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=28_000_000)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--trajectories", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--history-gib", type=float, default=16.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from hygeia_amd import _lib, single_group, synthetic

    dev = torch.device("cuda", 0)
    L = _lib.load()
    K, S, B, Nmax = 6, args.samples, args.trajectories, 250
    d = synthetic.simulate_device(args.sites, S, 1, K=K, coverage=100.0, omega=synthetic.SG_OMEGA, device=dev)
    meth, tot = d["meth_control"], d["tot_control"]
    del d
    sizes = [int(x) for x in synthetic.chromosome_sizes(args.sites)]
    begins = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    p = _lib.SgParams()
    L.hyg_sg_params_default(C.byref(p))
    assert p.n_regimes == K and p.num_particles_max == Nmax
    h = C.c_void_p()
    _lib.check(L.hyg_sg_model_create(C.byref(p), int(tot.to(torch.int32).max().item() & 0xFFFF), max(sizes),
                                     C.byref(h)))
    models = (C.c_void_p * 1)(h.value)
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    E = torch.empty((args.sites, K), dtype=torch.float64, device=dev)
    _lib.check(L.hyg_sg_emission(h, meth.data_ptr(), tot.data_ptr(), S, args.sites, E.data_ptr(), sp))
    budget = args.history_gib * 2 ** 30
    groups = single_group.history_groups(sizes, 1, Nmax, budget)
    cap_rows = max(sum(sizes[i] for i in g) for g in groups)
    h_lw = torch.empty((cap_rows, Nmax), dtype=torch.float64, device=dev)
    h_st = torch.empty((cap_rows, Nmax), dtype=torch.int32, device=dev)
    h_n = torch.empty((cap_rows,), dtype=torch.int32, device=dev)
    paths = torch.empty((cap_rows, B, 2), dtype=torch.int16, device=dev)
    hist = _lib.SgHistory(h_lw.data_ptr(), h_st.data_ptr(), h_n.data_ptr())

    def launch(which, idx):
        """One timed launch over the chromosomes idx (rows in that order): ms, log Z, status."""
        n = len(idx)
        arr = (_lib.SgChain * n)()
        row = 0
        for k, i in enumerate(idx):
            arr[k] = _lib.SgChain(begins[i], sizes[i], 0, 1, i, row)
            row += sizes[i]
        cm = (C.c_int32 * n)(*([0] * n))
        wsb = int(L.hyg_sg_filter_workspace_bytes_multi(models, 1, n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        log_z = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        st = torch.full((n,), 99, dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if which == "forward":
            _lib.check(L.hyg_sg_filter_chains_multi(models, 1, arr, cm, n, E.data_ptr(), ws.data_ptr(), wsb,
                                                    log_z.data_ptr(), None, None, None, st.data_ptr(), sp))
        elif which == "history":
            _lib.check(L.hyg_sg_history_chains_multi(models, 1, arr, cm, n, E.data_ptr(), ws.data_ptr(), wsb,
                                                     C.byref(hist), log_z.data_ptr(), None, None, None, st.data_ptr(),
                                                     sp))
        else:
            _lib.check(L.hyg_sg_sample_paths_multi(models, 1, arr, cm, n, C.byref(hist), None, B, paths.data_ptr(),
                                                   st.data_ptr(), sp))
        e1.record(stream)
        e1.synchronize()
        status = st.cpu().numpy()
        if (status != 0).any():
            raise RuntimeError(f"{which}: chains failed: {np.unique(status)}")
        ms = float(e0.elapsed_time(e1))
        print(f"[bench_sg_sample] {which} {n} chain(s), {row} sites: {ms:.1f} ms", file=sys.stderr, flush=True)
        return ms, log_z.cpu().numpy()

    out = {"workload": f"C2 single group, {args.sites} CpG, {S} samples jointly, K={K}, N_max={Nmax}, 1 seed, "
                       f"B={B} trajectories", "history_bytes_per_site": single_group.history_bytes(1, Nmax)}
    # ---- chr1: the longest chain alone, forward-only and history alternating
    c1 = int(np.argmax(sizes))
    launch("forward", [c1])  # warm-up of each build (code object load)
    launch("history", [c1])
    launch("sample", [c1])
    fwd, hst, smp = [], [], []
    for _ in range(args.repeats):
        ms, z0 = launch("forward", [c1])
        fwd.append(ms)
        ms, z1 = launch("history", [c1])
        hst.append(ms)
        if not np.array_equal(z0, z1):
            raise RuntimeError("the history launch's log Z differs from the forward-only launch's")
        smp.append(launch("sample", [c1])[0])
    T1 = sizes[c1]
    f, g, s = spread(fwd), spread(hst), spread(smp)
    out["chr1"] = {
        "sites": T1, "history_bytes": single_group.history_bytes(T1, Nmax),
        "forward_only": dict(f, us_per_step=f["median_ms"] * 1e3 / T1, spread_us_per_step=f["spread_ms"] * 1e3 / T1),
        "history": dict(g, us_per_step=g["median_ms"] * 1e3 / T1, spread_us_per_step=g["spread_ms"] * 1e3 / T1,
                        store_gbs=single_group.history_bytes(T1, Nmax) / (g["median_ms"] / 1e3) / 1e9),
        "history_minus_forward_us_per_step": (g["median_ms"] - f["median_ms"]) * 1e3 / T1,
        "sampler": s,
        "sampler_share_of_total": s["median_ms"] / (g["median_ms"] + s["median_ms"]),
    }
    # ---- genome: all 22 chains
    order = sorted(range(len(sizes)), key=lambda i: -sizes[i])
    gf = [launch("forward", order)[0] for _ in range(min(args.repeats, 2))]
    per_group = []
    for grp in groups:
        hm = launch("history", grp)[0]
        sm = launch("sample", grp)[0]
        per_group.append({"chromosomes": [i + 1 for i in grp], "sites": sum(sizes[i] for i in grp),
                          "history_ms": hm, "sampler_ms": sm})
    th, ts = sum(x["history_ms"] for x in per_group), sum(x["sampler_ms"] for x in per_group)
    out["genome"] = {
        "sites": args.sites, "history_bytes": single_group.history_bytes(args.sites, Nmax),
        "history_gib": args.history_gib, "groups": per_group,
        "forward_only_one_launch": spread(gf), "history_ms": th, "sampler_ms": ts,
        "sampler_share_of_total": ts / (th + ts),
    }
    L.hyg_sg_model_destroy(h)
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
