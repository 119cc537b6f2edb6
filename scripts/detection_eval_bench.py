"""Detection evaluation (tvc_roc_sweep): ms of the bootstrap sweep of B = 1 000 resamples at N = 10 000 / 100 000 / 1 000 000
scores, for the PHILOX source (draws made in the kernel) and the INDICES source (the caller's [B, N] draws), split into the sort
(``TVCEngine.roc_prepare``: finiteness check, stable sort, gathers) and the weights + sweep launch (``tvc_roc_sweep`` alone on the
prepared arrays), plus the whole ``bootstrap_metric("auc", ...)`` call as a user makes it.  The two smaller sizes run in the LDS
form (N <= ROC_LDS_ROWS) resp. the global form; the largest in the global form in chunks of the workspace budget.

Yardstick, timed in the same process where ``--host`` is given: the reference's loop (``roc_auc_score`` on ``labels[idx]``,
``scores[idx]`` per resample) on the host's threads (OMP_NUM_THREADS, 16 by default) over 64 resamples, scaled to 1 000.

One process, one warm-up per timing, medians of event-timed windows.  Run under a time limit:
    timeout 900 python scripts/detection_eval_bench.py [--host] [--small]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

pkg = importlib.import_module("multimodal-detection-consistency_amd")
_lib = pkg._lib
DEV = "cuda:0"
B = 1000


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


def sweep_call(eng, prepared, source, src, seed):
    """-> a function that launches tvc_roc_sweep of B rows on the prepared arrays into fixed outputs, and the outputs"""
    ss, sl, order = prepared
    dt = {"auc2": torch.int64, "auc": torch.float64, "ap": torch.float64, "youden_j": torch.float64}
    out = {n: torch.empty(B, dtype=dt.get(n, torch.int32), device=DEV) for n in _lib.ROC_OUT_FIELDS}
    o = _lib.RocOut(*[out[n].data_ptr() for n in _lib.ROC_OUT_FIELDS])
    rows = _lib.RocRows(ss.data_ptr(), sl.data_ptr(), order.data_ptr(), ss.numel(), source, 0 if src is None else src.data_ptr(), B, 0, seed)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        eng._check(eng.lib.tvc_roc_sweep(eng.handle, C.byref(rows), 0.95, None, 0, C.byref(o), stream))
    return run, out


def host_loop(scores, labels, resamples=64):
    from sklearn.metrics import roc_auc_score
    n = len(scores)
    threads = int(os.environ.get("OMP_NUM_THREADS", "16"))
    rng = np.random.default_rng(0)
    idx = [rng.integers(0, n, n) for _ in range(resamples)]
    roc_auc_score(labels[idx[0]], scores[idx[0]])
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        vals = list(ex.map(lambda i: roc_auc_score(labels[i], scores[i]), idx))
    dt = time.perf_counter() - t0
    return {"host_threads": threads, "host_resamples": resamples, "host_s": dt, "host_s_per_1000": dt * 1000 / resamples,
            "host_auc_mean": float(np.mean(vals))}


def size(eng, N, reps, host):
    g = torch.Generator(device=DEV).manual_seed(N)
    labels = (torch.rand(N, generator=g, device=DEV) < 0.3).to(torch.int64)
    scores = torch.randn(N, generator=g, device=DEV) + labels
    t_sort = median_ms(lambda: eng.roc_prepare(scores, labels), reps)
    prepared = eng.roc_prepare(scores, labels)
    res = {"N": N, "B": B, "form": "lds" if N <= eng.ROC_LDS_ROWS else "global", "sort_ms": t_sort[0], "sort_ms_min_max": t_sort[1:]}
    run, out = sweep_call(eng, prepared, _lib.TVC_ROC_SRC_PHILOX, None, 7)
    t = median_ms(run, reps)
    res.update(philox_sweep_ms=t[0], philox_sweep_ms_min_max=t[1:], philox_auc_mean=float(out["auc"].mean()),
               philox_ms_per_resample=t[0] / B)
    idx = torch.randint(0, N, (B, N), generator=g, device=DEV, dtype=torch.int32)
    run, out = sweep_call(eng, prepared, _lib.TVC_ROC_SRC_INDICES, idx, 0)
    t = median_ms(run, reps)
    res.update(indices_sweep_ms=t[0], indices_sweep_ms_min_max=t[1:], indices_auc_mean=float(out["auc"].mean()),
               indices_read_gbps=B * N * 4 / t[0] / 1e6)
    del idx
    t = median_ms(lambda: pkg.bootstrap_metric("auc", scores, labels, n_bootstrap=B, seed=7, engine=eng), max(1, reps // 2))
    d = pkg.bootstrap_metric("auc", scores, labels, n_bootstrap=B, seed=7, engine=eng)
    res.update(bootstrap_metric_auc_ms=t[0], auc_mean=float(d["mean"]), auc_lower=float(d["lower"]), auc_upper=float(d["upper"]))
    if host:
        res.update(host_loop(scores.cpu().numpy().astype(np.float64), labels.cpu().numpy()))
        res["speedup_vs_host"] = res["host_s_per_1000"] * 1e3 / (res["sort_ms"] + res["philox_sweep_ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="only N = 10 000 and 100 000")
    ap.add_argument("--host", action="store_true", help="also the sklearn loop on the host's threads at the two smaller sizes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detection_eval_bench.py measures on the GPU; none is visible")
    eng = pkg.TVCEngine(device=DEV)
    size(eng, 10000, 10, a.host)
    size(eng, 100000, 4, a.host)
    if not a.small:
        size(eng, 1000000, 2, False)
    eng.close()


if __name__ == "__main__":
    main()
