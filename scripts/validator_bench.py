"""The data validator's near-duplicate search on a bank slot (``TVCEngine.similar_pairs``: tvc_radius_graph at the widened
radius, tvc_graph_pair_count / tvc_graph_pair_fill, tvc_pair_cosine, the final filter): ms for the graph, for the pair list
(count, the host read of the total, fill), for the cosine of the nominated pairs and for the whole call, with the nominated
and the kept pair counts, at 10 000 x 512 on an fp32 slot and 100 000 x 768 on a bf16 slot, t = 0.95.  The rows are unit-norm
blobs of 100 rows around random unit centres with a per-row spread of 0.1 .. 0.3, so a blob's pairs lie on both sides of t.

Host baselines on the same rows at the 10 000-row shape only (where sklearn imports; BLAS and OpenMP on the host's threads):
``cosine_similarity`` plus ``np.argwhere(np.triu(S >= t, 1))`` -- a generous baseline, the pair walk vectorised -- and the
reference's literal double loop over i < j (src/evaluation/data_validator.py:407-415; --no-loop skips it: it takes a while).
Their pair lists are compared with the GPU's.

One process, one warm-up per shape, medians of event-timed windows.  Run under a time limit:
    timeout 900 python scripts/validator_bench.py [--small] [--no-loop]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

pkg = importlib.import_module("multimodal-detection-consistency_amd")
DEV = "cuda:0"
T = 0.95


def median_ms(fn, reps, windows=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def blobs(R, D, bf16):
    g = torch.Generator(device=DEV).manual_seed(R + D)
    K = max(2, R // 100)
    C = torch.nn.functional.normalize(torch.randn((K, D), generator=g, device=DEV), dim=1)
    X = torch.empty((R, D), dtype=torch.float32, device=DEV)
    for r0 in range(0, R, 1 << 16):
        n = min(1 << 16, R - r0)
        spread = 0.1 + 0.2 * torch.rand((n, 1), generator=g, device=DEV)
        X[r0:r0 + n] = C[torch.randint(K, (n,), generator=g, device=DEV)] + torch.randn((n, D), generator=g, device=DEV) * (spread / D ** 0.5)
    X = torch.nn.functional.normalize(X, dim=1)
    return X.bfloat16() if bf16 else X


def shape(eng, R, D, bf16, reps, host, loop):
    import math
    X = blobs(R, D, bf16)
    eng.set_bank(X, name="bench")
    eps = math.sqrt(2 - 2 * T + eng.similar_margin(D, T, bf16))
    adj, _ = eng.radius_graph(eps, bank="bench")
    nominated, _ = eng.graph_pairs(adj)
    pairs, sims = eng.similar_pairs(T, bank="bench")
    t_graph = median_ms(lambda: eng.radius_graph(eps, bank="bench"), reps)
    t_pairs = median_ms(lambda: eng.graph_pairs(adj), reps)
    t_cos = median_ms(lambda: eng.pair_cosine(nominated, bank="bench"), reps)
    t_all = median_ms(lambda: eng.similar_pairs(T, bank="bench"), reps)
    res = {"R": R, "D": D, "slot": "bf16" if bf16 else "fp32", "t": T, "eps2": eps * eps,
           "radius_graph_ms": t_graph[0], "radius_graph_ms_min_max": t_graph[1:], "graph_pairs_ms": t_pairs[0],
           "graph_pairs_ms_min_max": t_pairs[1:], "pair_cosine_ms": t_cos[0], "pair_cosine_ms_min_max": t_cos[1:],
           "similar_pairs_ms": t_all[0], "similar_pairs_ms_min_max": t_all[1:], "nominated_pairs": len(nominated), "pairs": len(pairs),
           "pair_cosine_gpairs_per_s": len(nominated) / t_cos[0] / 1e6 if len(nominated) else None, "adj_mib": adj.numel() * 4 / 2 ** 20}
    if host:
        try:
            from sklearn.metrics.pairwise import cosine_similarity
        except ImportError:
            res["host_vectorised_s"] = None
        else:
            Xh = X.float().cpu().numpy()
            got = pairs.cpu().numpy()
            t0 = time.perf_counter()
            S = cosine_similarity(Xh)
            want = np.argwhere(np.triu(S >= T, 1))
            res["host_vectorised_s"] = time.perf_counter() - t0
            res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS") or 16)
            # the host decides in fp32: pairs within a few ulps of t may differ
            same = len(want) == len(got) and bool((want == got).all())
            res["pairs_equal_host"] = same
            if not same:
                a, b = {tuple(p) for p in want.tolist()}, {tuple(p) for p in got.tolist()}
                res["pairs_only_host"], res["pairs_only_gpu"] = len(a - b), len(b - a)
                res["worst_disputed_margin"] = max((abs(float(S[i, j]) - T) for i, j in a ^ b), default=0.0)
            if loop:
                t0 = time.perf_counter()
                S = cosine_similarity(Xh)
                out = []
                for i in range(R):                                      # the reference's loop, literally
                    for j in range(i + 1, R):
                        similarity = S[i, j]
                        if similarity >= T:
                            out.append((i, j, similarity))
                res["host_double_loop_s"] = time.perf_counter() - t0
                res["double_loop_pairs"] = len(out)
    print(json.dumps(res), flush=True)
    eng.release_bank("bench")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="only the 10 000 x 512 shape")
    ap.add_argument("--no-loop", action="store_true", help="skip the reference's literal double loop on the host")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("validator_bench.py measures on the GPU; none is visible")
    eng = pkg.TVCEngine(device=DEV)
    shape(eng, 10000, 512, False, 20, True, not a.no_loop)
    if not a.small:
        shape(eng, 100000, 768, True, 3, False, False)
    eng.close()


if __name__ == "__main__":
    main()
