"""IVF search on a bank slot (tvc_ivf_probe / tvc_ivf_scan) against the flat exact search (tvc_bank_search) in the same
process: build time, ms per ivf_search and per bank_search at M in {1, 48, 4608} and nprobe in {1, 10, 32}, recall@10 of
the IVF result against the flat one, and the scan's bytes per second computed from shapes -- the rows of the probed lists
read once per list, plus the score buffer written by the scan and read by the select.  Shapes: R = 1 M x 768 on a bf16 slot
with nlist = 1 024 (scripts/build_faiss_indices.py's index) and R = 100 000 x 512 on an fp32 slot with nlist = 100
(retrieval_ref.py's).  Rows are unit vectors around 4 096 random directions, queries are bank rows with noise.

One process, one warm-up per measurement, medians of event-timed windows, the two searches alternating.  Run under a time
limit:
    timeout 900 python scripts/ivf_bench.py [--small]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

pkg = importlib.import_module("multimodal-detection-consistency_amd")
DEV = "cuda:0"


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating_ms(f, g, reps, windows=5):
    f(); g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(windows):
        tf.append(window_ms(f, reps))
        tg.append(window_ms(g, reps))
    return statistics.median(tf), statistics.median(tg)


def rows(R, D, dtype, g):
    centres = torch.nn.functional.normalize(torch.randn((4096, D), generator=g, device=DEV), dim=-1)
    X = torch.empty((R, D), dtype=dtype, device=DEV)
    for r0 in range(0, R, 1 << 17):
        n = min(1 << 17, R - r0)
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=DEV)] + 0.6 / D ** 0.5 * torch.randn((n, D), generator=g, device=DEV)
        X[r0:r0 + n] = torch.nn.functional.normalize(x, dim=-1)
    return X


def shape(eng, R, D, nlist, bf16, Ms, nprobes):
    g = torch.Generator(device=DEV).manual_seed(R + nlist)
    X = rows(R, D, torch.bfloat16 if bf16 else torch.float32, g)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ix = eng.ivf_build(X, nlist, "bench-ivf")
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    eng.set_bank(X, name="bench-flat")
    lens = (ix.offsets[1:] - ix.offsets[:-1]).long()
    row_bytes = D * 2 * (1 if bf16 else 2)
    print(json.dumps({"R": R, "D": D, "nlist": nlist, "slot": "bf16" if bf16 else "fp32", "build_s": build_s,
                      "max_list_rows": ix.max_list_rows, "mean_list_rows": R / nlist}), flush=True)
    for M in Ms:
        sel = torch.randint(0, R, (M,), generator=g, device=DEV)
        Q = torch.nn.functional.normalize(X[sel].float() + 0.3 / D ** 0.5 * torch.randn((M, D), generator=g, device=DEV), dim=-1)
        reps = 20 if M <= 48 else 3
        fidx, _, _ = eng.bank_search(Q, 10, want_moments=False, bank="bench-flat")
        eng.bank_status()
        for nprobe in nprobes:
            t_ivf, t_flat = alternating_ms(lambda: eng.ivf_search(Q, 10, nprobe, ix),
                                           lambda: eng.bank_search(Q, 10, want_moments=False, bank="bench-flat"), reps)
            t_probe = statistics.median(window_ms(lambda: eng.ivf_probe(Q, ix.centroids, nprobe), reps) for _ in range(3))
            idx, _, _ = eng.ivf_search(Q, 10, nprobe, ix)
            eng.bank_status()
            hit = (idx.unsqueeze(2) == fidx.unsqueeze(1)).any(2) & (idx >= 0)
            lists, _ = eng.ivf_probe(Q, ix.centroids, nprobe)
            lists = lists.long().clamp_(min=0)
            scan_bytes = float(lens[torch.unique(lists)].sum()) * row_bytes + 2.0 * 4 * float(lens[lists].sum())
            t_scan = max(t_ivf - t_probe, 1e-6)
            print(json.dumps({"R": R, "D": D, "nlist": nlist, "slot": "bf16" if bf16 else "fp32", "M": M, "nprobe": nprobe,
                              "ivf_search_ms": t_ivf, "probe_ms": t_probe, "flat_search_ms": t_flat, "speedup": t_flat / t_ivf,
                              "recall_at_10": float(hit.float().sum(1).mean() / 10), "scan_bytes": scan_bytes,
                              "scan_GBps": scan_bytes / t_scan / 1e6}), flush=True)
    eng.ivf_release(ix)
    eng.release_bank("bench-flat")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="only the 100 000 x 512 shape")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ivf_bench.py measures on the GPU; none is visible")
    eng = pkg.TVCEngine(device=DEV)
    if not a.small:
        shape(eng, 1000000, 768, 1024, True, (1, 48, 4608), (1, 10, 32))
    shape(eng, 100000, 512, 100, False, (1, 48, 4608), (1, 10, 32))
    eng.close()


if __name__ == "__main__":
    main()
