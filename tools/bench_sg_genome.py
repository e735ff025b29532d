"""A genome's single-group step 2 with per-chromosome models: one multi-model
launch against the alternatives.

Usage: python tools/bench_sg_genome.py [--sites 2800000] [--repeats 3] [--out FILE.json]

The chains are tools/bench_sg.py's C2 workload with the chromosome lengths
divided by 10 (back-to-back full-length launches would take minutes per
round): 22 chains over 2.8 M CpG sites, 4 samples jointly, K = 6, N_max = 250,
online parameter estimation with the flag defaults (ADAM, an update every 200
steps). Every chromosome starts from its own theta_0 ~ N(0, I) from a fixed
seed, as `estimate_parameters_and_regimes --estimate_parameters` starts each
task. The configurations run the same chains over the same counts; the timed
region is the emission table plus the chain launches, a host clock around work
that ends in a stream synchronise:

  a   one multi-model launch (hyg_sg_run_chains_pe_multi)
  b   one single-model launch per chromosome, back to back on one stream
  b1  the same launches from one host thread each, each on its own stream, with
      the machine's hardware-queue setting as it is
  c   one single-model launch with one theta_0 (the parameters' default) for
      all chains: bench_sg.py's shape, which per-chromosome theta_0 cannot use.
      It differs from a in theta_0 as well as in the kernels, and theta_0 moves
      the time either way, so it is d, not a, that c bounds
  d   a's launch with c's theta_0 as every model
  e   a cohort: 6 x 22 chains (the same counts six times, other seeds), each
      with its own model, in one launch; reported as sites/s

After one warm-up of each, the configurations alternate for --repeats rounds;
the line reports every time, the medians and the spread (max - min). The regime
probabilities and theta rows of a equal b's and b1's, and d's equal c's, bit
for bit (checked).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

THETA_SEED = 20260102
COHORT = 6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2_800_000)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="a,b,b1,c,d,e")
    ap.add_argument("--out", default=None, help="also write the result there (profiles/sg_genome_multi_model.json)")
    args = ap.parse_args()
    want = [x for x in args.configs.split(",") if x]

    import torch

    from hygeia_amd import _lib, synthetic

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L = _lib.load()
    K, S = 6, args.samples
    d = synthetic.simulate_device(args.sites, S, 1, K=K, coverage=100.0, omega=synthetic.SG_OMEGA, device=dev)
    meth, tot = d["meth_control"], d["tot_control"]
    sizes = synthetic.chromosome_sizes(args.sites)
    begins = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    n_chrom = len(sizes)
    order = sorted(range(n_chrom), key=lambda i: -int(sizes[i]))  # longest first
    max_reads = int(tot.to(torch.int32).max().item() & 0xFFFF)
    longest = int(max(sizes))
    rng = np.random.default_rng(THETA_SEED)
    thetas = [rng.standard_normal(K * K) for _ in range(COHORT * n_chrom)]

    def model(theta, max_duration=None):
        p = _lib.SgParams()
        L.hyg_sg_params_default(C.byref(p))  # pipeline defaults: K = 6, u = 3, N_max = 250, epsilon = 0.01
        if theta is not None:
            for j, v in enumerate(theta):
                p.theta[j] = float(v)
        h = C.c_void_p()
        _lib.check(L.hyg_sg_model_create(C.byref(p), max_reads, max_duration or longest + 10, C.byref(h)))
        return h

    # model m: chromosome m % 22 of cohort member m // 22, as long as its chromosome (the hazard tables of
    # 154 models are host work: on the host's threads)
    from concurrent.futures import ThreadPoolExecutor

    n_own = (COHORT if "e" in want else 1) * n_chrom
    with ThreadPoolExecutor(max_workers=int(os.environ.get("OMP_NUM_THREADS", "8"))) as pool:
        own = list(pool.map(lambda m: model(thetas[m], int(sizes[m % n_chrom]) + 10), range(n_own)))
    ceiling = model(None)
    same = [ceiling] * n_chrom  # 22 entries of the launch's table, one model
    pe = _lib.SgPeParams()
    L.hyg_sg_pe_params_default(C.byref(pe))
    every = pe.n_steps_without_update

    def chain_array(members):
        """The chains of `members` cohort members, longest first; chain k of member g
        writes rows g * sites + its chromosome's sites."""
        cs = [(g, i) for g in range(members) for i in order]
        cs.sort(key=lambda c: -int(sizes[c[1]]))
        arr = (_lib.SgChain * len(cs))()
        for k, (g, i) in enumerate(cs):
            arr[k] = _lib.SgChain(int(begins[i]), int(sizes[i]), 0, 1 + g, 0, g * args.sites + int(begins[i]))
        return arr, cs

    arr1, cs1 = chain_array(1)
    arr6, cs6 = chain_array(COHORT)
    rows1 = int(L.hyg_sg_pe_theta_rows(arr1, len(cs1), every))
    rows6 = int(L.hyg_sg_pe_theta_rows(arr6, len(cs6), every))
    hs = lambda hl: (C.c_void_p * len(hl))(*[h.value for h in hl])  # noqa: E731
    own1, own6, same1 = hs(own[:n_chrom]), hs(own), hs(same)
    cm1 = (C.c_int32 * len(cs1))(*[i for _, i in cs1])
    cm6 = (C.c_int32 * len(cs6))(*[g * n_chrom + i for g, i in cs6])
    wsb1 = int(L.hyg_sg_pe_workspace_bytes_multi(own1, n_chrom, arr1, len(cs1), 0))
    wsb6 = int(L.hyg_sg_pe_workspace_bytes_multi(own6, len(own), arr6, len(cs6), 0)) if "e" in want else 0
    if "e" not in want:
        arr6, cs6 = arr1, cs1
    ws = torch.empty(max(wsb1, wsb6), dtype=torch.uint8, device=dev)
    E = torch.empty((args.sites, K), dtype=torch.float64, device=dev)
    members = COHORT if "e" in want else 1
    f64 = dict(dtype=torch.float64, device=dev)
    probs = {k: torch.zeros((args.sites, K), **f64) for k in ("a", "b", "b1", "c", "d") if k in want}
    theta = {k: torch.zeros((rows1, K * K), **f64) for k in probs}
    if "e" in want:
        probs["e"], theta["e"] = torch.zeros((members * args.sites, K), **f64), torch.zeros((rows6, K * K), **f64)
    status = {k: torch.full((len(cs6 if k == "e" else cs1),), 99, dtype=torch.int32, device=dev) for k in probs}
    stream = torch.cuda.Stream(device=dev)
    sp = C.c_void_p(stream.cuda_stream)

    def emission():
        _lib.check(L.hyg_sg_emission(ceiling, meth.data_ptr(), tot.data_ptr(), S, args.sites, E.data_ptr(), sp))

    def multi(key, handles, n_models, arr, cm, n, wsb):
        emission()
        _lib.check(L.hyg_sg_run_chains_pe_multi(handles, n_models, C.byref(pe), arr, cm, n, E.data_ptr(),
                                                ws.data_ptr(), wsb, 0, probs[key].data_ptr(), theta[key].data_ptr(),
                                                status[key].data_ptr(), sp))

    # one launch per chromosome: chain k of arr1 alone, its theta rows where a's are
    row0 = np.concatenate([[0], np.cumsum([1 + (int(sizes[i]) - 1) // every for _, i in cs1])[:-1]])
    one = []
    for k, (_, i) in enumerate(cs1):
        a = (_lib.SgChain * 1)(arr1[k])
        one.append((a, own[i], int(L.hyg_sg_pe_workspace_bytes(own[i], a, 1, 0)), int(row0[k]), k))

    def single(key, a, h, wsb, r0, k, wsp, strm):
        _lib.check(L.hyg_sg_run_chains_pe(h, C.byref(pe), a, 1, E.data_ptr(), wsp, wsb, 0, probs[key].data_ptr(),
                                          theta[key][r0:].data_ptr(), status[key][k:].data_ptr(), strm))

    def run_b():
        emission()
        for (a, h, wsb, r0, k) in one:
            single("b", a, h, wsb, r0, k, ws.data_ptr(), sp)

    ws_b1, streams_b1 = [], []
    if "b1" in want:
        ws_b1 = [torch.empty(wsb, dtype=torch.uint8, device=dev) for (_, _, wsb, _, _) in one]
        streams_b1 = [torch.cuda.Stream(device=dev) for _ in one]

    def run_b1():
        emission()
        stream.synchronize()  # the chains' streams read the table
        errs = []

        def work(j):
            try:
                a, h, wsb, r0, k = one[j]
                single("b1", a, h, wsb, r0, k, ws_b1[j].data_ptr(), C.c_void_p(streams_b1[j].cuda_stream))
                streams_b1[j].synchronize()
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(j,)) for j in range(len(one))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if errs:
            raise errs[0]

    def run_c():
        emission()
        wsb = int(L.hyg_sg_pe_workspace_bytes(ceiling, arr1, len(cs1), 0))
        _lib.check(L.hyg_sg_run_chains_pe(ceiling, C.byref(pe), arr1, len(cs1), E.data_ptr(), ws.data_ptr(), wsb, 0,
                                          probs["c"].data_ptr(), theta["c"].data_ptr(), status["c"].data_ptr(), sp))

    runs = {"a": lambda: multi("a", own1, n_chrom, arr1, cm1, len(cs1), wsb1), "b": run_b, "b1": run_b1, "c": run_c,
            "d": lambda: multi("d", same1, n_chrom, arr1, cm1, len(cs1), wsb1),
            "e": lambda: multi("e", own6, len(own), arr6, cm6, len(cs6), wsb6)}

    def timed(fn) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    for k in want:  # warm-up
        print(f"warm-up {k}: {timed(runs[k]):.1f} ms", file=sys.stderr, flush=True)
    ms = {k: [] for k in runs}
    for r in range(args.repeats):
        for k in want:
            ms[k].append(timed(runs[k]))
            print(f"round {r} {k}: {ms[k][-1]:.1f} ms", file=sys.stderr, flush=True)
    torch.cuda.synchronize(dev)
    for k in probs:
        if (status[k] != 0).any().item():
            raise RuntimeError(f"chains of {k} failed: {status[k].unique().tolist()}")
    for x, y in (("a", "b"), ("a", "b1"), ("d", "c")):
        if x in probs and y in probs and not (torch.equal(probs[x], probs[y]) and torch.equal(theta[x], theta[y])):
            raise RuntimeError(f"{x} and {y} differ")
    if "a" in probs and "c" in probs and torch.equal(theta["a"], theta["c"]):
        raise RuntimeError("a ran with c's theta")

    def stats(v, units):
        if not v:
            return {"ms": []}  # not run (--configs)
        med = float(np.median(v))
        return {"ms": [round(x, 2) for x in v], "median_ms": round(med, 2), "spread_ms": round(max(v) - min(v), 2),
                "sites_per_s": round(units / (med / 1000.0))}

    med = lambda k: float(np.median(ms[k])) if ms[k] else None  # noqa: E731
    ratio = lambda x, y: round(med(x) / med(y), 3) if ms[x] and ms[y] else None  # noqa: E731
    # two-sided: the two configurations' [min, max] ranges of times share a point
    overlap = lambda x, y: (bool(min(ms[x]) <= max(ms[y]) and min(ms[y]) <= max(ms[x]))  # noqa: E731
                            if ms[x] and ms[y] else None)
    diff = lambda x, y: round(med(x) - med(y), 2) if ms[x] and ms[y] else None  # noqa: E731
    line = {
        "tool": "tools/bench_sg_genome.py", "device": torch.cuda.get_device_name(dev),
        "source_hash": __import__("hygeia_amd.build", fromlist=["source_hash"]).source_hash(),
        "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
        "workload": f"C2 / 10: {args.sites} CpG over {n_chrom} chromosome chains (longest {longest}), {S} samples "
                    f"jointly, K={K}, N_max=250, online parameter estimation (ADAM, every {every}); theta_0 ~ N(0, I) "
                    f"per chromosome (seed {THETA_SEED})",
        "timed_region": "emission + chain launches, host clock to stream synchronise; 1 warm-up of each, then "
                        f"{args.repeats} alternating rounds",
        "total_over_longest_sites": round(args.sites / longest, 2),
        "a_one_multi_model_launch": stats(ms["a"], args.sites),
        "b_one_launch_per_chromosome": stats(ms["b"], args.sites),
        "b1_one_thread_and_stream_per_chromosome": stats(ms["b1"], args.sites),
        "c_one_theta_single_launch": stats(ms["c"], args.sites),
        "d_multi_model_launch_with_c_theta": stats(ms["d"], args.sites),
        "e_cohort_one_launch": dict(stats(ms["e"], COHORT * args.sites), chains=len(cs6), models=len(own)),
        "b_over_a_median": ratio("b", "a"), "b1_over_a_median": ratio("b1", "a"),
        "a_over_c_median": ratio("a", "c"), "d_over_c_median": ratio("d", "c"),
        "a_times_overlap_c": overlap("a", "c"), "a_minus_c_median_ms": diff("a", "c"),
        "d_times_overlap_c": overlap("d", "c"), "d_minus_c_median_ms": diff("d", "c"),
        "outputs_a_equal_b": "a" in probs and "b" in probs, "outputs_a_equal_b1": "a" in probs and "b1" in probs,
        "outputs_d_equal_c": "d" in probs and "c" in probs,
    }
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)
            fh.write("\n")
    for h in own + [ceiling]:
        L.hyg_sg_model_destroy(h)


if __name__ == "__main__":
    main()
