"""Forward-only launches against the full launch, on the C3 chains.

Usage: python tools/bench_filter.py [--sites 28000000] [--repeats 3] [--out profiles/filter_bench.json]

The chains are bench.py's C3 workload (hg38-proportioned chromosomes, 100 k
segments + 5 k buffers, 2 seeds, 4 + 4 samples, K = 6, M = 50, B = 25: 582
chains, 56 M site-seeds). Counts and the emission table stay resident; the
timed region is the chain launch alone (a host clock around work that ends in
a stream synchronise), and the forward kernel's own time comes from the HIP
events of hyg_set_kernel_timing. Five configurations:

  a  the forward-only launch of the chains (hyg_tg_filter_chains): log Z, no
     history, no backward
  b  the full single-model launch of the same chains (hyg_tg_run_chains)
  c  a grid of 9 settings (3 omega_case x 3 split_prob) over a genome's
     per-chromosome theta as ONE forward-only multi-model launch
     (hyg_tg_filter_chains_multi): 9 x the chains of a, models (chromosome) x
     (setting)
  d  the traced forward-only launch of the chains of a with log Z_t alone
     (hyg_tg_trace_chains, trace="log_z": one more store per step)
  e  the same with all three arrays (trace="all": log Z_t and the filtering
     marginals, the class sums of every step)

After one warm-up of each, the configurations alternate (a, b, c, d, e, a, ...) for
--repeats rounds. The line reports every time, medians and spreads (max -
min), the two sizing functions' workspace bytes, and checks that a's log Z
equals b's bit for bit.
"""
from __future__ import annotations

import argparse
import ctypes
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETA_SEED = 20260101
OMEGAS, SPLITS = (0.7, 0.8, 0.9), (0.005, 0.01, 0.05)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=28_000_000)
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--theta-sd", type=float, default=0.3, help="per-chromosome N(0, sd) added to uniform_theta (c)")
    ap.add_argument("--configs", default="abcde")
    ap.add_argument("--out", default=None, help="also write the result there (profiles/filter_bench.json)")
    args = ap.parse_args()

    import torch

    from hygeia_amd import _lib, synthetic, two_group

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.load()
    K, M, B = 6, 50, 25
    data = synthetic.simulate_device(args.sites, args.samples, args.samples, K=K, coverage=100.0, device=dev)
    sizes = synthetic.chromosome_sizes(args.sites)
    segs = synthetic.segment_chains(sizes)
    n_chrom = len(sizes)
    # (chromosome, chain) longest first, as bench.py orders a launch
    allc = sorted(((ci, (s0, n, sd, (ci << 32) | b)) for sd in range(args.seeds)
                   for (ci, b, s0, n, r0, rl) in segs), key=lambda c: -c[1][1])
    units = args.seeds * sum(rl for (ci, b, s0, n, r0, rl) in segs)
    chains, n_out = [], 0
    for _, (s0, n, sd, cid) in allc:
        chains.append((s0, n, sd, cid, n_out))
        n_out += n
    steps = n_out
    max_reads = int(max(data["tot_control"].to(torch.int32).max().item() & 0xFFFF,
                        data["tot_case"].to(torch.int32).max().item() & 0xFFFF))
    mu, sg = synthetic.regime_params(K)
    uniform = two_group.uniform_theta(K, 0.8)
    longest = max(c[1] for c in chains)
    kw = dict(num_resampled_ancestors=M, num_samples_backward=B, max_total_reads=max_reads, max_duration=longest)
    model = two_group.CaseControlModel(mu, sg, uniform, **kw)
    # c: (chromosome theta) x (setting) models, task x seed x setting chains, longest first
    rng = np.random.default_rng(THETA_SEED)
    thetas = [uniform + rng.normal(0.0, args.theta_sd, uniform.shape) for _ in range(n_chrom)]
    settings = list(itertools.product(OMEGAS, SPLITS))
    grid_models = [two_group.CaseControlModel(mu, sg, th, omega_case=om, split_prob=sp, **kw)
                   for th in thetas for (om, sp) in settings] if "c" in args.configs else []
    grid_chains = [c for c in chains for _ in settings]
    grid_index = [ci * len(settings) + s for ci, _ in allc for s in range(len(settings))]

    ws_filter = two_group.DeviceFilter.workspace_bytes(model, chains)
    ws_full = two_group.DeviceChains.workspace_bytes(model, chains)
    ws_grid = two_group.DeviceFilter.workspace_bytes(grid_models, grid_chains) if grid_models else None
    df_a = two_group.DeviceFilter(model, chains, device=dev)
    dc_b = two_group.DeviceChains(model, chains, n_out, device=dev) if "b" in args.configs else None
    df_c = (two_group.DeviceFilter(grid_models, grid_chains, device=dev, chain_model=grid_index)
            if grid_models else None)
    df_d = (two_group.DeviceFilter(model, chains, device=dev, trace="log_z", n_out_rows=n_out)
            if "d" in args.configs else None)
    df_e = (two_group.DeviceFilter(model, chains, device=dev, trace="all", n_out_rows=n_out)
            if "e" in args.configs else None)
    stream = torch.cuda.Stream(device=dev)
    sp_ = stream.cuda_stream
    E = df_a.emission(data["meth_control"], data["tot_control"], data["meth_case"], data["tot_case"], stream=sp_)
    stream.synchronize()

    def timed(fn) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    runs = {"a": lambda: df_a.run(E, stream=sp_), "b": lambda: dc_b.run(E, stream=sp_),
            "c": lambda: df_c.run(E, stream=sp_), "d": lambda: df_d.run(E, stream=sp_),
            "e": lambda: df_e.run(E, stream=sp_)}
    configs = [k for k in "abcde" if k in args.configs]
    if "a" not in configs:
        raise SystemExit("--configs must hold a")
    L.hyg_set_kernel_timing(1)
    ms3 = (ctypes.c_float * 3)()
    for k in configs:  # warm-up: every kernel the timed rounds use
        timed(runs[k])
    ms = {k: [] for k in "abcde"}
    fwd = {k: [] for k in "abcde"}
    bwd = []
    for r in range(args.repeats):
        for k in configs:
            ms[k].append(timed(runs[k]))
            _lib.check(L.hyg_tg_last_kernel_ms(ms3))
            fwd[k].append(float(ms3[1]))
            if k == "b":
                bwd.append(float(ms3[2]))
            elif ms3[2] != -1.0:
                raise RuntimeError("a forward-only launch reported a backward kernel time")
            print(f"round {r} {k}: {ms[k][-1]:.1f} ms (forward kernel {ms3[1]:.1f} ms)", file=sys.stderr, flush=True)
    L.hyg_set_kernel_timing(0)
    for d in (df_a, dc_b, df_c, df_d, df_e):
        if d is not None and (d.status != 0).any().item():
            raise RuntimeError("chains failed")
    for d in (df_d, df_e):  # a traced launch: the plain launch's log Z, and its own last row
        if d is not None:
            lz = d.log_z.cpu().numpy()
            last = d.log_z_t.cpu().numpy()[[c[4] + c[1] - 1 for c in chains]]
            if lz.tobytes() != df_a.log_z.cpu().numpy().tobytes() or last.tobytes() != lz.tobytes():
                raise RuntimeError("a traced launch's log Z differs from the forward-only launch's")
    if df_d is not None and df_e is not None and not torch.equal(df_d.log_z_t, df_e.log_z_t):
        raise RuntimeError("log Z_t differs between the two traced launches")
    if dc_b is not None and df_a.log_z.cpu().numpy().tobytes() != dc_b.log_z.cpu().numpy().tobytes():
        raise RuntimeError("a chain's log Z differs between the forward-only and the full launch")

    def stats(v, n_units=units):
        if not v:
            return {"ms": []}  # not run (--configs)
        return {"ms": [round(x, 2) for x in v], "median_ms": round(float(np.median(v)), 2),
                "spread_ms": round(max(v) - min(v), 2),
                "site_seeds_per_s": round(n_units / (float(np.median(v)) / 1000.0))}

    def name(fn, *a):
        buf = ctypes.create_string_buffer(96)
        fn(*a, buf, 96)
        return buf.value.decode()

    a, b, c = fwd["a"], fwd["b"], fwd["c"]
    med = lambda v: float(np.median(v))  # noqa: E731

    def traced(k, df, what):
        if df is None:
            return {"ms": []}
        r = dict(stats(ms[k]), trace=what, kernel=name(L.hyg_tg_trace_kernel_name, model.handle, len(chains)),
                 forward_kernel_ms=stats(fwd[k]),
                 output_bytes=sum(int(t.numel() * t.element_size())
                                  for t in (df.log_z_t, df.split_probs, df.regime_probs) if t is not None),
                 forward_over_a_forward_median=round(med(fwd[k]) / med(a), 4),
                 within_a_spread=bool(min(a) <= med(fwd[k]) <= max(a)))
        if b:
            r["launch_over_b_launch_median"] = round(med(ms[k]) / med(ms["b"]), 4)
        return r

    line = {
        "tool": "tools/bench_filter.py", "device": torch.cuda.get_device_name(dev),
        "source_hash": __import__("hygeia_amd.build", fromlist=["source_hash"]).source_hash(),
        "workload": f"C3 chains: {args.sites} CpG over {n_chrom} chromosomes, 100k segments + 5k buffers, "
                    f"{args.samples}+{args.samples} samples, K={K}, M={M}, B={B}, {args.seeds} seeds, "
                    f"{len(chains)} chains, {steps} steps",
        "timed_region": "the chain launch on a resident emission table, host clock to stream synchronise; 1 warm-up "
                        f"of each, then {args.repeats} alternating rounds {', '.join(configs)}",
        "units_site_seeds": units,
        "workspace_bytes": {"forward_only": ws_filter, "full_launch": ws_full, "grid_forward_only": ws_grid},
        "a_forward_only": dict(stats(ms["a"]), kernel=name(L.hyg_tg_filter_kernel_name, model.handle, len(chains)),
                               forward_kernel_ms=stats(a)),
        "b_full_launch": dict(stats(ms["b"]), kernel=name(L.hyg_tg_kernel_name, model.handle, len(chains), 0),
                              forward_kernel_ms=stats(b), backward_kernel_ms=stats(bwd)),
        "c_grid_forward_only_multi_model": dict(
            stats(ms["c"], units * len(settings)), settings=len(settings), models=len(grid_models),
            chains=len(grid_chains), omega_case=OMEGAS, split_prob=SPLITS,
            kernel=(name(L.hyg_tg_filter_kernel_name_multi, df_c._handles, len(grid_models), len(grid_chains))
                    if df_c is not None else None),
            forward_kernel_ms=stats(c, units * len(settings))),
        "d_traced_log_z": traced("d", df_d, "log_z"),
        "e_traced_all": traced("e", df_e, "all"),
        # e's forward less d's: what the class sums (and their two stores per step) cost, as a share of e's forward
        "class_sum_share_of_e_forward": round((med(fwd["e"]) - med(fwd["d"])) / med(fwd["e"]), 4)
        if fwd["d"] and fwd["e"] else None,
        "a_forward_over_b_forward_median": round(float(np.median(a) / np.median(b)), 4) if b else None,
        "a_over_b_launch_median": round(float(np.median(ms["a"]) / np.median(ms["b"])), 4) if b else None,
        "c_per_setting_over_a_median": round(float(np.median(ms["c"]) / len(settings) / np.median(ms["a"])), 4)
        if c else None,
        "log_z_a_equals_b": bool(b) or None,
    }
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)
            fh.write("\n")
    for m in grid_models + [model]:
        m.close()


if __name__ == "__main__":
    main()
