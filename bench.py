#!/usr/bin/env python3
"""bench.py -- defended queries/sec of the TVC hot path on MI355X.

A "step" is one pass of the hot path over one batch of synthetic queries with
inputs resident in HBM: encode B images + B*(N+1) token rows with the HIP CLIP
towers, exact top-k search of all B*(N+2) embedding rows against the bank,
per-query consistency scores, records copied to the host.  Default workload =
BASELINE.json configs[2]: ViT-L/14 bf16, B=512, N=8, 1M-row bank, one GPU.

    python bench.py --gpus N --steps K --warmup W          # N > 1: starts N ranks itself
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step` = one
timed step).  --full adds everything else the line can carry: the profile pass (roofline, per-kernel
times), the live HBM-traffic passes, the extras (other precisions, API rates, PGD, SD, ...) and the CPU
baselines.  --dump-outputs DIR writes what the last timed step returned as DIR/<name>.npy.

Multi-GPU (one process per GPU, torch.distributed backend nccl = RCCL over xGMI):
  * default: queries are data-parallel (encoders + bank replicated per GPU, no
    collective on the data path) -> "scaling": "weak";
  * --shard-bank (BASELINE configs[3]): --bank-rows is the GLOBAL bank, row-sharded
    over the ranks; all-gather of the query rows + all-to-all of partial top-k lists.
Rank 0 prints ONE JSON line.  With --gpus N > 1 and no WORLD_SIZE in the environment
this process never touches the GPU: it starts `python -m torch.distributed.run` with N
fresh worker processes, forwards their output and exits with their code (replaces
src/utils/multi_gpu_processor.py:494-620 at the driver's entry point).
"""
import argparse
import importlib
import json
import math
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_BF16_DENSE_TFLOPS = 2500.0     # /opt/skills/guides/MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="ViT-L/14")
    p.add_argument("--batch", type=int, default=512, help="queries per GPU per step")
    p.add_argument("--variants", type=int, default=8)
    p.add_argument("--bank-rows", type=int, default=None,
                   help="bank rows (default 1 000 000 = configs[2]; 10 000 000 with --shard-bank = configs[3])")
    p.add_argument("--full", action="store_true",
                   help="also run everything beyond the headline figure: the profile pass (roofline, per-kernel times), the "
                        "live HBM-traffic passes, the extras and the CPU baselines (default: set up, warm up, time the steps, "
                        "print the line)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last step returned as DIR/<name>.npy (float32 / float64)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    p.add_argument("--cpu-seconds", type=float, default=20.0)
    p.add_argument("--no-extras", action="store_true",
                   help="--full: skip the extra measurements of the N=1 run (dense-text rate, through-the-API rates, "
                        "reference-schedule / 1-thread / configs[0] CPU baselines)")
    p.add_argument("--no-profile-pass", action="store_true", help="--full: skip the profile pass (roofline)")
    p.add_argument("--shard-bank", action="store_true",
                   help="BASELINE configs[3]: --bank-rows is the GLOBAL bank, row-sharded over the ranks; "
                        "partial top-k lists are exchanged with RCCL (all-gather + all-to-all) and merged on the GPU")
    p.add_argument("--exchange", default="fused", choices=["fused", "two_phase", "single_phase"],
                   help="--shard-bank: how the partial lists travel (sharding.py); fused = one fixed-size all-to-all, "
                        "no host synchronisation, pipelined under the next batch's towers (default)")
    p.add_argument("--rehearse-one-gpu", action="store_true",
                   help="multi-rank rehearsal on a ONE-GPU box: every rank uses cuda:0 and the process group is "
                        "gloo (RCCL refuses two ranks on one device); checks the launch contract, not speed")
    p.add_argument("--serial-towers", action="store_true",
                   help="encode text then images on ONE stream (default: two streams, the towers overlap)")
    p.add_argument("--chunk-images", type=int, default=0, help="images per tower pass (0 = library default)")
    p.add_argument("--no-prefix-sharing", action="store_true",
                   help="encode every variant in full (default: variants share the rows of the token prefix they have "
                        "in common with their original - bit-identical, see TVC_OPT_TEXT_GROUP)")
    p.add_argument("--dense-text", action="store_true",
                   help="run the text tower on all 77 positions (disable EOT packing)")
    p.add_argument("--unplanted-bank", action="store_true",
                   help="pure Gaussian bank (no row reaches the 0.3 threshold, the reference branch of the consistency "
                        "kernel sees no references); default: neighbours of the text rows are planted")
    p.add_argument("--no-live-traffic", action="store_true",
                   help="do not measure roofline.traffic live (two rocprofv3 --pmc child passes of this command with --steps 1, "
                        "run BEFORE this process touches the GPU; a --full N=1 run does, ~1.5 min); fall back to the committed profile")
    p.add_argument("--sd-model", default="runwayml/stable-diffusion-v1-5",
                   help="latent-diffusion geometry of the sd_reference extra: the reference's default (src/sd_ref.py:221) or "
                        "'stabilityai/stable-diffusion-2-1-base' (src/__init__.py:110-113)")
    p.add_argument("--no-parity-modes", action="store_true", help="skip the parity_mode extra (the step in the split-bf16 and fp32 tower modes)")
    p.add_argument("--master-port", type=int, default=0)
    p.add_argument("--dry-run-launch", action="store_true",
                   help="launch-contract rehearsal WITHOUT a GPU (CPU test of the --gpus N launcher): the ranks form a "
                        "gloo group, run the barrier + max-over-ranks reduction and rank 0 prints a line with "
                        '"dry_run": true and value 0 -- never a measurement')
    a = p.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    if not a.full:
        a.no_cpu_baseline = a.no_extras = a.no_profile_pass = a.no_live_traffic = True
    if a.bank_rows is None:
        a.bank_rows = 10_000_000 if a.shard_bank else 1_000_000
    return a


# --------------------------------------------------------------------------- launcher
def launch_ranks(a) -> int:
    """`python bench.py --gpus N` without a torchrun environment: start N worker ranks (fresh processes; this
    parent has not initialised the GPU), stream their output, return their exit code."""
    import torch
    have = torch.cuda.device_count()            # counting devices does not initialise the GPU on this image
    if not a.rehearse_one_gpu and not a.dry_run_launch and have < a.gpus:
        print(f"bench.py: --gpus {a.gpus} but only {have} GPU(s) are visible", file=sys.stderr)
        return 3
    port = a.master_port or (29500 + os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True)
    line = None
    for ln in proc.stdout:
        if ln.lstrip().startswith('{"metric"'):
            line = ln
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if line is None:
        print(f"bench.py: the {a.gpus}-rank run produced no result line (exit code {rc})", file=sys.stderr)
        return rc or 4
    try:
        n = json.loads(line).get("n_gpus")
    except Exception:
        n = None
    if n != a.gpus:
        print(f"bench.py: asked for {a.gpus} ranks, the result line says n_gpus={n}", file=sys.stderr)
        return rc or 5
    sys.stdout.write(line)
    sys.stdout.flush()
    return rc


# --------------------------------------------------------------------------- live HBM traffic (PMC)
def measure_traffic_live(a):
    """roofline.traffic measured IN THIS RUN: two child processes `rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE -- python3 bench.py
    --steps 1 ...` (separate passes, counters only, the program itself after `--`), started before this process touches
    the GPU.  Corrections as /opt/skills/guides/MI355X_MICROARCH.md (HBM): KB counters; on gfx950 FETCH_SIZE tallies the
    128-byte requests of wide reads at 64 B (x2; calibrated on a launch of known bytes: profiles/r03_pmc_calibration.json),
    WRITE_SIZE exact.  Returns {kernel: {launches, hbm_MB_per_launch}} or None (no rocprofv3 / a pass failed)."""
    import collections, csv, glob, re, shutil, tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    tmp = tempfile.mkdtemp(prefix="tvc_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    base = [sys.executable, str(Path(__file__).resolve()), "--steps", "1", "--warmup", "1", "--serial-towers", "--no-cpu-baseline",
            "--no-extras", "--no-profile-pass", "--no-live-traffic", "--model", a.model, "--batch", str(a.batch),
            "--variants", str(a.variants), "--bank-rows", str(a.bank_rows)]
    per = {}
    try:
        for counter, tag in (("FETCH_SIZE", "f"), ("WRITE_SIZE", "w")):
            cmd = [exe, "--pmc", counter, "-d", os.path.join(tmp, tag), "-o", tag, "--output-format", "csv", "--"] + base
            r = subprocess.run(cmd, env=env, cwd=str(ROOT), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=150)
            files = glob.glob(os.path.join(tmp, tag, "**", f"{tag}_counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                print(f"bench.py: live traffic pass {counter} failed (rc {r.returncode}, files {files}); using the committed profile", file=sys.stderr)
                return None
            tot, disp = collections.defaultdict(float), collections.defaultdict(set)
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] != counter:
                    continue
                name = re.sub(r"\(.*", "", row["Kernel_Name"]).replace("void ", "").strip()
                tot[name] += float(row["Counter_Value"]); disp[name].add(row["Dispatch_Id"])
            per[tag] = {k: (tot[k] / len(disp[k]), len(disp[k])) for k in tot}
    except Exception as ex:
        print(f"bench.py: live traffic measurement failed ({type(ex).__name__}: {ex}); using the committed profile", file=sys.stderr)
        return None
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for k, (fkb, n) in per["f"].items():
        if k in per["w"] and not k.startswith("at::") and "rocclr" not in k:
            out[k] = {"launches": n, "hbm_MB_per_launch": round((2 * fkb + per["w"][k][0]) / 1024, 1)}
    return out


def host_cpus() -> int:
    """CPUs this process may actually use: min(affinity, cgroup cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


# --------------------------------------------------------------------------- CPU baselines (oracle = checker / timed port)
def cpu_baseline(arch, weights, images, tokens, bank_cpu, budget_s, threads, schedule="dedup", max_queries=None, scores_out=None):
    """The oracle (CPU restatement of the reference path, PyTorch-CPU fp32 towers + numpy scores) timed on
    this box's host cores on a bounded sample of the same workload.
    schedule "dedup": image encoded once per query, the N+1 texts in one batch (the de-duplicated minimum);
    schedule "reference": the reference's own schedule, src/detector.py:461-471 + :573 -- one image forward and
    one text forward per get_text_image_similarity call (N+1 for the variants method, one more for the
    consistency method), i.e. N+2 image-tower passes per query."""
    import torch
    from oracle import clip_oracle, tvc_oracle
    vw, tw = weights
    torch.set_num_threads(threads)

    def one(i):
        with torch.no_grad():
            if schedule == "dedup":
                fi = clip_oracle.vision_forward(vw, images[i:i + 1], arch.vision.heads, arch.patch)
                ft = clip_oracle.text_forward(tw, tokens[i], arch.text.heads)
            else:
                fis, fts = [], []
                for n in list(range(tokens.shape[1])) + [0]:          # N+1 similarity calls + the consistency call
                    fis.append(clip_oracle.vision_forward(vw, images[i:i + 1], arch.vision.heads, arch.patch))
                    fts.append(clip_oracle.text_forward(tw, tokens[i, n:n + 1], arch.text.heads))
                fi, ft = fis[0], torch.cat(fts[:-1])
        return tvc_oracle.detect_batch(fi.numpy(), ft.numpy()[None], bank_cpu)

    if schedule == "dedup" and threads > 1:
        one(0)                  # warm-up (thread pools, allocator)
    t0 = time.perf_counter()
    done = 0
    limit = images.shape[0] if max_queries is None else min(max_queries, images.shape[0])
    while done < limit:
        r = one(done)
        if scores_out is not None:          # the oracle's scores of query `done` (parity_mode: deviation of each tower mode)
            scores_out.append({k: float(r[k][0]) for k in ("original_similarity", "score_src", "overall_exp")})
        done += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    return done / dt, done, dt


# --------------------------------------------------------------------------- synthetic strings for the API-level runs
class WordReplaceVariants:
    """Variant generator for the through-the-API measurement: replaces ceil(0.3 * words) words of the
    caption in place (``synonym_replacement_ratio`` 0.3, src/text_augment.py:57) -- the string-level
    twin of ``synth.make_tokens``, so both measurements see the same token statistics."""

    def __init__(self, n, vocab, seed=5):
        import random
        self.n, self.vocab, self.rng = n, vocab, random.Random(seed)

    def generate_variants(self, text):
        words = text.split()
        out = []
        for _ in range(self.n):
            w = list(words)
            for p in self.rng.sample(range(len(w)), int(math.ceil(0.3 * len(w)))):
                w[p] = self.rng.choice(self.vocab)
            out.append(" ".join(w))
        return out


def dump_outputs(out_dir, rec, img_idx, n_variants, lib):
    """--dump-outputs: what the last timed step returned to its caller (rank 0's queries), split as
    detector.unpack_records splits the records (layout: include/tvc.h); integer words as exact float64."""
    import numpy as np
    r = rec.numpy()
    h, M = lib.TVC_REC_HEAD + n_variants, lib.TVC_REC_MAXREF
    arrays = {
        "record_scores": r[:, :h],                                                        # head words + variant similarities
        "record_reference_indices": np.ascontiguousarray(r[:, h:h + M]).view(np.int32).astype(np.float64),
        "record_reference_similarities": r[:, h + M:h + 2 * M],
        "image_topk_indices": img_idx.numpy().astype(np.float64),                         # bank rows nearest each image
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, x in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(x))


def make_captions(n, seed=3):
    import random
    rng = random.Random(seed)
    vocab = [f"w{i}" for i in range(4000)]
    return [" ".join(rng.choice(vocab) for _ in range(rng.randint(5, 20))) for _ in range(n)], vocab


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a))

    # PMC passes run as child processes BEFORE anything here touches the GPU (--full N=1 run of the default workload only)
    live_traffic = None
    if (int(os.environ.get("WORLD_SIZE", "1")) == 1 and not a.no_live_traffic and not a.no_extras and not a.no_profile_pass
            and not a.shard_bank and not a.dry_run_launch):
        t_pm = time.perf_counter()
        live_traffic = measure_traffic_live(a)
        if live_traffic is not None:
            live_traffic["_seconds"] = round(time.perf_counter() - t_pm, 1)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.dry_run_launch:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
        t = torch.tensor([1e-3 * (rank + 1)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        line = {"metric": "defended queries/sec", "value": 0.0, "unit": "queries/s", "n_gpus": world,
                "steps": a.steps, "warmup": a.warmup, "dry_run": True, "max_over_ranks_s": float(t.item()),
                "distributed": {"backend": dist.get_backend(), "world_size": dist.get_world_size()}}
        if a.shard_bank:
            # the sharded layout's collectives on stand-in tensors (no kernels): row split, all-gather of query rows, the
            # fixed-size all-to-all, the status all-reduce -- the shapes of one configs[3] step divided by 1 000
            sh = importlib.import_module("multimodal-detection-consistency_amd.sharding")
            lo, hi = sh.shard_bounds(a.bank_rows, world, rank)
            m, D = 8, 16
            rows = torch.full((m, D), float(rank))
            allrows = torch.empty((world * m, D))
            dist.all_gather_into_tensor(allrows, rows)
            send = torch.arange(world, dtype=torch.float32).view(world, 1).repeat(1, 4) + 100.0 * rank
            recv = torch.empty_like(send)
            sh._all_to_all(recv, send, None)
            ok = bool((allrows.view(world, m, D)[:, 0, 0] == torch.arange(world)).all()) and \
                bool((recv[:, 0] == 100.0 * torch.arange(world) + rank).all())
            sizes = torch.tensor([float(hi - lo), 1.0 if ok else 0.0], dtype=torch.float64)
            gathered = [torch.empty_like(sizes) for _ in range(world)]
            dist.all_gather(gathered, sizes)
            line["shard_rows"] = [int(g[0]) for g in gathered]
            line["collectives_ok"] = all(bool(g[1] > 0) for g in gathered)
        if rank == 0:
            print(json.dumps(line), flush=True)
        dist.destroy_process_group()
        return
    pkg = importlib.import_module("multimodal-detection-consistency_amd")
    if world != a.gpus and rank == 0:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; reporting n_gpus={world}", file=sys.stderr)
    if a.rehearse_one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1 or a.shard_bank:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        if a.rehearse_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)

    arch = pkg.get_arch(a.model)
    B, N, R, D = a.batch, a.variants, a.bank_rows, arch.embed_dim
    weights = pkg.synth.make_clip_weights(arch, seed=0)
    clip = pkg.CLIPModel(pkg.CLIPConfig(model_name=a.model, device=str(dev)), weights=weights)
    eng = clip.engine
    images = pkg.synth.make_images(B, arch.image_size, seed=1 + rank).to(dev)
    tokens = pkg.synth.make_tokens(B, N, arch.ctx, seed=2 + 1000 * rank).to(dev)
    if a.shard_bank:
        lo, hi = pkg.sharding.shard_bounds(R, world, rank)
        bank = pkg.synth.make_bank(hi - lo, D, seed=7 + rank, device=str(dev), dtype=torch.bfloat16)
    else:
        bank = pkg.synth.make_bank(R, D, seed=7, device=str(dev), dtype=torch.bfloat16)
    if not a.unplanted_bank and bank.shape[0] >= 4 * B * (N + 1):
        # neighbours of this rank's text rows (cos 0.45 .. 0.99): retrieval keeps references above the 0.3
        # threshold, so the de-duplication / cos(image, reference) branch of the consistency kernel runs
        ft0 = eng.encode_text(tokens.view(B * (N + 1), arch.ctx))
        bank = pkg.synth.plant_neighbours(bank, ft0.cpu(), per_anchor=1, seed=11 + rank)
        del ft0
    if a.shard_bank:
        # "fused": ONE fixed-size all-to-all per step, no host read-back inside the search (sharding.py)
        sharded = pkg.sharding.ShardedBankSearch(pkg.sharding.HipShardOps(eng, lo, 0.3),
                                                 rows_per_shard=(R + world - 1) // world, mode=a.exchange)
    eng.set_bank(bank)
    if a.dense_text:
        eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 0)
    if a.chunk_images:
        eng.set_option(pkg._lib.TVC_OPT_MAX_CHUNK_IMAGES, a.chunk_images)
    cfg = pkg.ConsistencyConfig()
    k = max(cfg.search_k, cfg.reference_count)

    s_img, s_txt = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def towers():
        """Both towers of one batch on their own streams; returns (fi, ft, event that marks both done)."""
        main = torch.cuda.current_stream()
        s_txt.wait_stream(main); s_img.wait_stream(main)
        with torch.cuda.stream(s_txt):
            ft = eng.encode_text(tokens.view(B * (N + 1), arch.ctx), group=0 if a.no_prefix_sharing else N + 1)
        with torch.cuda.stream(s_img):
            fi = eng.encode_image(images)
        return fi, ft

    pipe_state = {}

    def step_sharded_pipelined():
        """--shard-bank, fused exchange: nothing between the towers and the records reads a value back, so the host
        enqueues batch i + 1's towers (their own streams) BEFORE batch i's search / exchange / consistency (main stream):
        the all-gather and the all-to-all of batch i run under the towers of batch i + 1.  One step =
        one batch retired; the pipeline is primed in the warm-up and drained by the closing synchronize."""
        main = torch.cuda.current_stream()
        if "next" not in pipe_state:
            pipe_state["next"] = towers()
        fi, ft = pipe_state["next"]
        main.wait_stream(s_txt); main.wait_stream(s_img)          # batch i's embeddings are ready for the main stream
        pipe_state["next"] = towers()                             # batch i + 1: enqueued now, runs beside what follows
        rows = torch.cat([fi, ft])
        idx, sim, feat = sharded.search(rows, k, cfg.reference_count, feat_from=B)
        rec = eng.consistency(fi, ft.view(B, N + 1, D), cfg, idx[B:].contiguous(), sim[B:].contiguous(), feat[B:].contiguous())
        out = rec.cpu(), idx[:B].cpu()
        sharded.check_status()            # once per step, INSIDE the timed region: every rank's overflow flag, all-reduced
        return out

    def step_dp_pipelined():
        """The data-parallel step software-pipelined like `step_sharded_pipelined`: batch i + 1's towers are enqueued on their
        own streams BEFORE batch i's bank search / consistency on the main stream, so the MFMA-bound filter and the
        latency-bound select / consistency kernels of batch i run beside the row kernels of batch i + 1.  One step = one batch
        retired (records on the host); primed in the warm-up, drained by the closing synchronize.  A reported extra
        (`pipelined`), never `value`: the headline step is one batch end to end."""
        main = torch.cuda.current_stream()
        if "next_dp" not in pipe_state:
            pipe_state["next_dp"] = towers()
        fi, ft = pipe_state["next_dp"]
        main.wait_stream(s_txt); main.wait_stream(s_img)
        pipe_state["next_dp"] = towers()
        rows = torch.cat([fi, ft])
        idx, sim, _ = eng.bank_search(rows, k, cfg.similarity_threshold, want_moments=False)
        tidx, tsim = idx[B:], sim[B:]
        feat = eng.bank_gather(tidx[:, :cfg.reference_count].contiguous())
        rec = eng.consistency(fi, ft.view(B, N + 1, D), cfg, tidx.contiguous(), tsim.contiguous(), feat)
        return rec.cpu(), idx[:B].cpu()

    def step(serial=False):
        if a.shard_bank and a.exchange == "fused" and not serial and not a.serial_towers:
            return step_sharded_pipelined()
        if a.serial_towers or serial:
            ft = eng.encode_text(tokens.view(B * (N + 1), arch.ctx), group=0 if a.no_prefix_sharing else N + 1)   # first: its one row-count read-back
            fi = eng.encode_image(images)                               # happens while the GPU is still idle
        else:
            # The towers are independent until the bank search: run them on two streams.  The HBM-bound
            # row kernels / attention of one tower then overlap the MFMA-bound GEMMs of the other, and
            # a GEMM's last partial round of tiles no longer leaves CUs idle.
            main = torch.cuda.current_stream()
            s_txt.wait_stream(main); s_img.wait_stream(main)
            with torch.cuda.stream(s_txt):
                ft = eng.encode_text(tokens.view(B * (N + 1), arch.ctx), group=0 if a.no_prefix_sharing else N + 1)
            with torch.cuda.stream(s_img):
                fi = eng.encode_image(images)
            main.wait_stream(s_txt); main.wait_stream(s_img)
        rows = torch.cat([fi, ft])                                  # M = B*(N+2) query-side rows
        if a.shard_bank:
            # every rank searches ALL ranks' rows on its shard; partials go back to the rows' owners
            idx, sim, feat = sharded.search(rows, k, cfg.reference_count, feat_from=B)    # image rows need no reference rows
            rec = eng.consistency(fi, ft.view(B, N + 1, D), cfg, idx[B:].contiguous(), sim[B:].contiguous(),
                                  feat[B:].contiguous())
            out = rec.cpu(), idx[:B].cpu()
            if a.exchange == "fused":
                sharded.check_status()    # the other exchange modes are status-checked per call
            return out
        idx, sim, _ = eng.bank_search(rows, k, cfg.similarity_threshold, want_moments=False)
        tidx, tsim = idx[B:], sim[B:]
        feat = eng.bank_gather(tidx[:, :cfg.reference_count].contiguous())
        rec = eng.consistency(fi, ft.view(B, N + 1, D), cfg, tidx.contiguous(), tsim.contiguous(), feat)
        return rec.cpu(), idx[:B].cpu()

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            out = fn()
        if not a.shard_bank:
            eng.bank_status()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        sync()
        return time.perf_counter() - t0, out

    dt, (rec, img_idx) = timed(step, a.steps, a.warmup)
    if world > 1:
        t = torch.tensor([dt], device="cpu" if a.rehearse_one_gpu else dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if not a.shard_bank:
        eng.bank_status()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, rec, img_idx, N, pkg._lib)
    assert torch.isfinite(rec[:, :11]).all()      # words >= 12+N hold int32 bit patterns (-1 = NaN bits)
    kept_refs = float(rec[:, 8].mean())           # references kept per query by the consistency kernel

    roof = None
    prof = None
    if not a.no_profile_pass:
        # separate pass with HIP events around every launch (not part of the timed region)
        eng.profile_begin()
        step(serial=True)       # one stream: kernel durations not inflated by the other tower's kernels
        prof = eng.profile_end()
        g = prof["gemm"]
        achieved = g["work"] / (g["ms"] * 1e-3) / 1e12 if g["ms"] > 0 else 0.0
        roof = {"bound": "mfma", "kernel": "gemm_ring4_kernel<EPI> (all tvc GEMM launches of a step: the persistent ring kernels + the few small gemm_bf16_kernel ones)", "achieved": round(achieved, 2),
                "peak": PEAK_BF16_DENSE_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_DENSE_TFLOPS, 4),
                "traffic": None, "launches_per_step": g["launches"],
                "avg_launch_ms": round(g["ms"] / max(g["launches"], 1), 4),
                # the denominator of `traffic`: COMPULSORY HBM bytes per launch (every distinct operand plane read once, the
                # output written once) of the same launches -- the GEMM launches of >= 64 tiles, i.e. the ring kernels
                "traffic_algorithmic": round(g["big_bytes"] / max(g["big_launches"], 1) / 1e9, 3),
                "ring_launches_per_step": g["big_launches"]}

    if roof is not None and rank == 0 and live_traffic:
        ring = [(v["launches"], v["hbm_MB_per_launch"]) for kk, v in live_traffic.items() if kk.startswith("gemm_ring")]
        if ring:
            roof["traffic"] = round(sum(n * mb for n, mb in ring) / sum(n for n, _ in ring) / 1e3, 3)
            roof["traffic_unit"] = "GB per launch (PMC: 2 x FETCH_SIZE + WRITE_SIZE, launch-weighted mean over the ring GEMMs)"
            if roof.get("traffic_algorithmic"):
                roof["traffic_over_algorithmic"] = round(roof["traffic"] / roof["traffic_algorithmic"], 2)
            roof["traffic_source"] = (f"live: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; counters only) of this command with "
                                      f"--steps 1, run by bench.py as child processes before the timed run ({live_traffic.get('_seconds')} s)")
            roof["traffic_by_kernel_GB"] = {kk: round(v["hbm_MB_per_launch"] / 1e3, 3) for kk, v in live_traffic.items()
                                            if isinstance(v, dict) and (kk.startswith("gemm_ring") or kk.startswith("layernorm") or
                                                                        kk.startswith("attention_kernel<17") or kk.startswith("bank_filter"))}
    if roof is not None and rank == 0 and roof.get("traffic") is None:
        # HBM bytes per launch of the dominant kernel family when the live PMC passes did not run (--no-live-traffic, no
        # rocprofv3): a static figure from the committed rocprofv3 --pmc summary of this same command
        try:
            import glob
            here = os.path.dirname(os.path.abspath(__file__))
            files = sorted(glob.glob(os.path.join(here, "profiles", "*hbm_traffic_pmc.json")))
            if files and a.model == "ViT-L/14" and B == 512 and N == 8 and R == 1_000_000 and not a.shard_bank:
                pm = json.load(open(files[-1]))
                ring = [(v["launches"], v["hbm_MB_per_launch_corrected"]) for kk, v in pm.items()
                        if kk.startswith("gemm_ring")]
                if ring:
                    roof["traffic"] = round(sum(n * mb for n, mb in ring) / sum(n for n, _ in ring) / 1e3, 3)
                    roof["traffic_unit"] = "GB per launch (PMC, launch-weighted mean over the ring GEMMs)"
                    roof["traffic_source"] = "static (from committed profile): profiles/" + os.path.basename(files[-1])
        except Exception:       # a missing / unreadable summary leaves traffic null
            pass

    out = None
    if rank == 0:
        qps = world * B * a.steps / dt
        flops_q = arch.flops_image() + (N + 1) * arch.flops_text() + 2.0 * (N + 2) * R * D
        # executed MFMA work of one step (the text tower runs on the packed rows only; the bank GEMM
        # multiplies two bf16 planes per query row)
        exec_flops = None
        if prof:
            exec_flops = prof["gemm"]["work"] + prof["attention"]["work"] + prof["bank"]["work"]
        if a.shard_bank:
            wl = (f"{a.model} bf16, batch={B}/GPU, N={N} variants, {R}-row bf16 bank row-sharded over {world} GPU(s) "
                  f"({-(-R // world)} rows each), encode + exact top-{k} search with RCCL all-gather / all-to-all of partial "
                  f"lists + consistency (BASELINE configs[3])")
        else:
            tag = "BASELINE configs[2]" if (a.model, B, N, R) == ("ViT-L/14", 512, 8, 1_000_000) else \
                  "BASELINE configs[1]" if (a.model, B, N, R) == ("ViT-B/32", 256, 4, 100_000) else "custom"
            wl = (f"{a.model} bf16, batch={B}/GPU, N={N} variants, {R}-row bf16 bank, "
                  f"encode + exact top-{k} bank search + consistency ({tag})")
        out = {
            "metric": "defended queries/sec", "value": round(qps, 2), "unit": "queries/s", "n_gpus": world,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(1e3 * dt / a.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "config": {"workload": wl,
                       "global_batch": world * B, "parallelism": (f"dp{world} queries x bank rows sharded {world}-way (RCCL all-gather + all-to-all of partial top-k; exchange={a.exchange}"
                                                       + (", pipelined under the next batch's towers" if a.exchange == "fused" and not a.serial_towers else "") + ")"
                                       if a.shard_bank else f"dp{world}"),
                       "text_packing": "dense-77" if a.dense_text else ("eot-packed" + ("" if a.no_prefix_sharing else " + variant prefix sharing") + " (bit-identical, see DESIGN.md)"),
                       "bank": "gaussian" if a.unplanted_bank else "gaussian + planted neighbours of the text rows",
                       "references_kept_per_query": round(kept_refs, 2),
                       "algorithmic_gflop_per_query_dense": round(flops_q / 1e9, 2),
                       "executed_gflop_per_query": round(exec_flops / B / 1e9, 2) if exec_flops else None,
                       "executed_path_tflops": round(qps * exec_flops / B / 1e12, 1) if exec_flops else None},
            "roofline": roof,
        }
        if prof:
            out["kernel_ms_per_step"] = {c: round(v["ms"], 2) for c, v in prof.items()}
            bk = prof["bank"]
            if bk["ms"] > 0:
                out["bank_stage"] = {"mfma_tflops": round(bk["work"] / (bk["ms"] * 1e-3) / 1e12, 1),
                                     "bank_stream_GBps": round(bank.shape[0] * D * 2 / (bk["ms"] * 1e-3) / 1e9, 1)}

    if rank == 0 and a.shard_bank:
        out["exchange"] = dict(sharded.last_exchange)
        out["exchange"]["status_check"] = ("check_status() once per step inside the timed region: the local overflow flag read back + "
                                           "one all_reduce(MAX) of two floats" if a.exchange == "fused" else "per call (status-checked search)")
    if rank == 0 and dist.is_initialized():
        # what the process group itself reports -- so that a SCALE record shows RCCL (backend "nccl" on ROCm) really saw N ranks
        out["distributed"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                              "ranks_on_distinct_gpus": not a.rehearse_one_gpu,
                              "data_path_collectives": ("all_gather_into_tensor + all_to_all_single per step (bank rows sharded)"
                                                        if a.shard_bank else "none (data-parallel queries, replicated bank)"),
                              "timing": "barrier + synchronize on both sides, MAX over ranks (all_reduce)"}
    extras = world == 1 and not a.no_extras and not a.shard_bank
    if extras and not a.dense_text:
        # the same workload with the text tower on all 77 positions (no EOT packing): the rate does not
        # depend on caption length
        eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 0)
        d2, _ = timed(step, max(2, min(a.steps, 5)), 1)
        eng.set_option(pkg._lib.TVC_OPT_TEXT_PACKING, 1)
        out["dense_text_qps"] = round(B * max(2, min(a.steps, 5)) / d2, 2)
    if extras and not a.serial_towers:
        ks = max(2, min(a.steps, 10))
        d_pl, (rec_pl, _) = timed(step_dp_pipelined, ks, 2)
        torch.cuda.synchronize()
        pipe_state.pop("next_dp", None)
        assert torch.equal(rec_pl.view(torch.int32), rec.view(torch.int32))      # same batch, bit-identical records (the pipeline changes the schedule only; bitwise: the index words are NaN patterns as floats)
        out["pipelined"] = {"qps": round(B * ks / d_pl, 2), "ms_per_step": round(d_pl / ks * 1e3, 3),
                            "note": "the same step software-pipelined: batch i + 1's towers enqueued before batch i's bank "
                                    "search / consistency (one batch retired per step, records bit-identical); not `value`"}
    rec_modes = {"bf16": rec}
    if extras and not a.no_parity_modes:
        # ---- the two fp32-grade tower modes on the SAME step (BASELINE.json: scores within 1e-4 of the reference's fp32 CPU
        # path): "split" = hi | lo bf16 planes, three MFMA products (TVC_OPT_TOWER_PRECISION = 2); "fp32" = the exact-f32
        # matrix instruction (= 1).  Their deviation from the CPU oracle is filled in below, from the queries the
        # cpu_baseline leg runs anyway.  Never `value`.
        out["parity_mode"] = {}
        for mode, ks in (("split", 3), ("fp32", 1)):
            eng.set_precision(mode)
            d_m, (rec_m, _) = timed(lambda: step(serial=False), ks, 1)
            rec_modes[mode] = rec_m
            out["parity_mode"][mode] = {"tower_precision_option": eng.PRECISIONS[mode], "qps": round(B * ks / d_m, 2),
                                        "ms_per_step": round(d_m / ks * 1e3, 2), "vs_bf16_step": round(d_m / ks / (dt / a.steps), 2)}
        eng.set_precision("bf16")
    if extras:
        # ---- the same workload through the API the reference's runners call: strings + image tensors in,
        # Python result objects out (experiments/runners/run_detection.py:164-203, run_ablation.py:308-312)
        texts, vocab = make_captions(B)
        gen = WordReplaceVariants(N, vocab)
        pipe = pkg.MultiModalDetectionPipeline(
            pkg.PipelineConfig(enable_sd_reference=False,
                               detector_config=pkg.DetectorConfig(clip_model=a.model, num_text_variants=N)),
            clip_model=clip, text_augmenter=gen)
        pipe.retriever.set_image_features(bank)                     # the retriever's own bank slot (same rows)
        defense = pkg.MultiModalDefenseDetector(clip, config=pkg.DetectionConfig(text_variant_count=N),
                                                text_generator=gen)
        defense.set_reference_bank(bank)
        ks = max(2, min(a.steps, 5))
        d_pipe, res = timed(lambda: pipe.detect(images=images, texts=texts, return_details=True), ks, 1)
        assert len(res["scores"]) == B
        d_def, res = timed(lambda: defense.batch_detect(images, texts), ks, 1)
        assert len(res) == B
        out["through_api"] = {
            "pipeline_detect_qps": round(B * ks / d_pipe, 2), "defense_batch_detect_qps": round(B * ks / d_def, 2),
            "engine_level_qps": out["value"],
            "note": "strings + device image tensors in, Python result objects out; pipeline.detect = text_augment + "
                    "retrieval (B texts re-encoded + top-5 of the 1M-row index) + detection (src polarity, no bank); "
                    "defense.batch_detect = encode + bank search of the B*(N+1) text rows + consistency + the stateful "
                    "host-side ConsistencyChecker"}
        # one query at a time, as the reference's own callers do (src/pipeline.py:284-288 -> process_single): latency
        lat = []
        for i in range(6):
            torch.cuda.synchronize(); t1 = time.perf_counter()
            pipe.process_single(images[i], texts[i])
            torch.cuda.synchronize(); lat.append(time.perf_counter() - t1)
        out["through_api"]["process_single_ms"] = round(sorted(lat[1:])[len(lat[1:]) // 2] * 1e3, 2)
        out["through_api"]["process_single_note"] = ("median of 5 calls, one query end to end (text variants + retrieval over the "
                                                     f"{R}-row index + detection, no SD references); the reference's README quotes 19.1 ms "
                                                     "P50 / 45.7 ms P99 per query and 52.3 queries/s for its full pipeline (Qwen + SD) on "
                                                     "6 x RTX 4090 (README.md:890-898): other hardware and workload, context only")

    if extras:
        # ---- K5 in the HBM-bound regime of SURVEY.md 8(d): small query batches (the reference searches one query at a time,
        # src/retrieval.py:636-680; configs[0] has 48 rows).  GB/s = R * D * 2 B / t of the whole search (sample pre-pass,
        # filter, select), against the ~6.3 TB/s a streaming kernel reaches on this chip.
        sm = {}
        qrows = torch.nn.functional.normalize(torch.randn((256, D), device=dev, generator=torch.Generator(device=dev).manual_seed(5)), dim=-1)
        for Ms in (1, 10, 48, 256):
            q = qrows[:Ms].contiguous()
            for _ in range(3):
                eng.bank_search(q, k, cfg.similarity_threshold, want_moments=False)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                eng.bank_search(q, k, cfg.similarity_threshold, want_moments=False)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 20
            sm[f"M={Ms}"] = {"ms": round(ms, 3), "GBps": round(bank.shape[0] * D * 2 / ms / 1e6, 1),
                             "frac_of_6.3TBps": round(bank.shape[0] * D * 2 / ms / 1e6 / 6300, 3)}
        eng.bank_status()
        sm["note"] = (f"exact top-{k} of M query rows over the {bank.shape[0]}-row bf16 bank, whole search per call; M <= 64 takes the "
                      "skinny filter (bank.hip: bank_filter_skinny_kernel), larger batches the 256-query-tile ring kernel")
        out["bank_stage_small_m"] = sm

    if extras and not a.serial_towers:
        # ---- the same step when the caller holds HOST buffers (pinned): H2D of the 512 images (308 MB fp32) and the
        # tokens inside the timed region, each on its tower's stream so that the text copy + tower overlap the image
        # copy.  A reported extra -- never `value` (inputs resident in HBM).
        h_img, h_tok = images.cpu().pin_memory(), tokens.cpu().pin_memory()
        d_img, d_tok = torch.empty_like(images), torch.empty_like(tokens)

        def step_host():
            main = torch.cuda.current_stream()
            s_txt.wait_stream(main); s_img.wait_stream(main)
            with torch.cuda.stream(s_txt):
                d_tok.copy_(h_tok, non_blocking=True)
                ft = eng.encode_text(d_tok.view(B * (N + 1), arch.ctx), group=0 if a.no_prefix_sharing else N + 1)
            with torch.cuda.stream(s_img):
                d_img.copy_(h_img, non_blocking=True)
                fi = eng.encode_image(d_img)
            main.wait_stream(s_txt); main.wait_stream(s_img)
            rows = torch.cat([fi, ft])
            idx, sim, _ = eng.bank_search(rows, k, cfg.similarity_threshold, want_moments=False)
            tidx, tsim = idx[B:], sim[B:]
            feat = eng.bank_gather(tidx[:, :cfg.reference_count].contiguous())
            rec2 = eng.consistency(fi, ft.view(B, N + 1, D), cfg, tidx.contiguous(), tsim.contiguous(), feat)
            return rec2.cpu(), idx[:B].cpu()

        ks = max(2, min(a.steps, 5))
        d_host, _ = timed(step_host, ks, 1)
        out["host_inputs_qps"] = round(B * ks / d_host, 2)
        out["host_inputs_note"] = (f"pinned host images ({images.numel() * 4 / 1e6:.0f} MB) + tokens copied H2D inside the timed "
                                   f"region, per step: {d_host / ks * 1e3:.1f} ms")
        del h_img, h_tok, d_img, d_tok

    if extras:
        # ---- the attack inner loop: forward + input gradient + projected sign step per image,
        # at the same tower, batch 32 (src/attacks/pgd_attack.py:42) -- an extra line, not the headline metric
        pb = min(32, B)
        clean = images[:pb].contiguous()
        adv, mom = clean.clone(), torch.zeros_like(clean)
        tf = eng.encode_text(tokens[:pb, 0].contiguous())
        g_out = (tf / pb).contiguous()

        def pgd_iter():
            eng.encode_image_grad(adv, True)
            g = eng.encode_image_backward(g_out)
            eng.pgd_step(adv, clean, g, mom, 8 / 255, 2 / 255, 0.9, 0.0, 1.0, False)

        ks = 10
        eng.profile_begin()
        pgd_iter(); sync()
        prof = eng.profile_end()
        d_pgd, _ = timed(pgd_iter, ks, 2)
        fwd_flop = prof["gemm"]["work"] / pb
        out["pgd_inner_loop"] = {"image_steps_per_s": round(pb * ks / d_pgd, 1), "batch": pb, "ms_per_step": round(d_pgd / ks * 1e3, 2),
                                 "gemm_tflops_in_step": round(prof["gemm"]["work"] / (prof["gemm"]["ms"] * 1e-3) / 1e12, 1),
                                 "gemm_gflop_per_image_step": round(fwd_flop / 1e9, 1),
                                 "note": "forward (the backward's inputs are kept, nothing is recomputed) + the four dX GEMMs per layer; no weight gradients"}
        # two batches of 32 in flight, each on its own stream and engine handle (what PGDAttacker.perturb does by default,
        # PGDAttackConfig.concurrent_batches = 2): every batch computed as it is alone
        try:
            eng2 = pkg.TVCEngine(arch, weights[0], None, device=str(dev))
            clean2 = images[pb:2 * pb].contiguous() if B >= 2 * pb else clean.clone()
            adv2, mom2 = clean2.clone(), torch.zeros_like(clean2)
            jobs = [(eng, s_img, adv, clean, mom), (eng2, s_txt, adv2, clean2, mom2)]

            def pgd_iter2():          # no join between steps: each batch runs its own loop (timed() ends on a device-wide sync)
                for e_, st_, adv_, clean_, mom_ in jobs:
                    with torch.cuda.stream(st_):
                        e_.encode_image_grad(adv_, True)
                        g_ = e_.encode_image_backward(g_out)
                        e_.pgd_step(adv_, clean_, g_, mom_, 8 / 255, 2 / 255, 0.9, 0.0, 1.0, False)

            sync()
            d2, _ = timed(pgd_iter2, ks, 2)
            sync()
            out["pgd_inner_loop"]["two_batches_in_flight"] = {"image_steps_per_s": round(2 * pb * ks / d2, 1), "batch": pb,
                                                              "ms_per_step_pair": round(d2 / ks * 1e3, 2)}
            eng2.close()
            del adv2, mom2, clean2
        except Exception as ex:       # an extra: never the reason a bench run fails
            out["pgd_inner_loop"]["two_batches_in_flight"] = {"error": f"{type(ex).__name__}: {ex}"}

    if extras and B >= 256 and a.model == "ViT-L/14":
        # ---- the same inner loop at a full chip: batch 256 (the reference's 32 is a default of PGDAttackConfig, not a
        # constraint of PGDAttacker.perturb; the kept activations are 31 GB of the 288 GB)
        pb = 256
        clean = images[:pb].contiguous()
        adv, mom = clean.clone(), torch.zeros_like(clean)
        g_out = (eng.encode_text(tokens[:pb, 0].contiguous()) / pb).contiguous()

        def pgd_iter256():
            eng.encode_image_grad(adv, True)
            g = eng.encode_image_backward(g_out)
            eng.pgd_step(adv, clean, g, mom, 8 / 255, 2 / 255, 0.9, 0.0, 1.0, False)

        eng.profile_begin()
        pgd_iter256(); sync()
        prof = eng.profile_end()
        d_pgd, _ = timed(pgd_iter256, 5, 1)
        out["pgd_inner_loop_b256"] = {"image_steps_per_s": round(pb * 5 / d_pgd, 1), "batch": pb, "ms_per_step": round(d_pgd / 5 * 1e3, 2),
                                      "gemm_tflops_in_step": round(prof["gemm"]["work"] / (prof["gemm"]["ms"] * 1e-3) / 1e12, 1)}
        del adv, mom, clean

    if extras and a.model == "ViT-L/14":
        # ---- bank construction (scripts/build_faiss_indices.py:59-120 benchmarks its own QPS): the image
        # tower streaming synthetic images at B = 512 -> L2-normalised rows -> features.npy in the reference's layout
        import tempfile
        import numpy as np
        n_img = 100 * B if B >= 256 else 20 * B
        with tempfile.TemporaryDirectory() as td:
            feats = np.lib.format.open_memmap(os.path.join(td, "features.npy"), mode="w+", dtype=np.float32, shape=(n_img, D))
            pin = torch.empty((B, D), dtype=torch.float32).pin_memory()
            sync()
            t0 = time.perf_counter(); t_write = 0.0
            prev = None
            for b0 in range(0, n_img, B):
                f = eng.encode_image(images)                      # (the same synthetic batch: content does not change the cost)
                if prev is not None:
                    tw = time.perf_counter()
                    feats[prev[0]:prev[0] + B] = prev[1].cpu().numpy()       # batch i - 1 lands while batch i computes
                    t_write += time.perf_counter() - tw
                prev = (b0, f)
            tw = time.perf_counter()
            feats[prev[0]:prev[0] + B] = prev[1].cpu().numpy()
            feats.flush()
            t_write += time.perf_counter() - tw
            d_build = time.perf_counter() - t0
        out["bank_build"] = {"images_per_s": round(n_img / d_build, 1), "images": n_img, "batch": B, "seconds": round(d_build, 2),
                             "writer_share": round(t_write / d_build, 3),
                             "note": "ViT-L/14 image tower at B=512 -> L2-normalised fp32 rows -> features.npy (np.lib.format memmap); "
                                     "writer_share = host time inside the D2H copy + file write (mostly waiting for the GPU)"}

    if extras and a.model == "ViT-L/14" and not os.environ.get("TVC_BENCH_NO_SD"):
        # ---- SD reference generation (BASELINE configs[4]): prompts x seeds denoised together, 20 PNDM
        # steps (experiments/defenses/generative_ref.py:24) at 64 x 64 latents, guidance 7.5, VAE decode to 512 x 512,
        # device-side preprocessing, ONE image-tower launch -> reference embeddings
        torch.cuda.empty_cache()
        sd = pkg.StableDiffusionModel(pkg.SDModelConfig(model_name=a.sd_model, device=str(dev), random_init=True), clip_model=clip)
        n_img, steps_sd = 12, 20
        prompts = [f"a photo of object number {i}" for i in range(n_img)]
        seeds_sd = list(range(n_img))

        def sd_step():
            imgs = sd.generate_batch(prompts, seeds_sd, steps_sd, 7.5, 512, 512)
            return eng.encode_image(clip.preprocess_tensor(imgs), True)

        sd_eng = sd.text_engine
        sd_step(); sync()
        # the category times come from a pass with the two guidance halves on ONE stream (TVC_OPT_SD_STREAMS = 1): with two
        # streams the launches of the halves overlap and an event pair around a launch also spans the other half's kernels
        sd_eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 1)
        d_sd1, _ = timed(sd_step, 1, 1)
        eng.profile_begin()
        sd_step(); sync()
        prof = eng.profile_end()
        sd_eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 2)
        d_sd, _ = timed(sd_step, 2, 1)
        gemm_tf = prof["gemm"]["work"] / (prof["gemm"]["ms"] * 1e-3) / 1e12 if prof["gemm"]["ms"] > 0 else 0.0
        # the same generator at a batch that fills the chip's low-resolution levels (80 samples: the 8 x 8 level's 32 token
        # tiles x 5 feature tiles, the 16 x 16 level's 255): every image is bit-identical to the one the 12-image batch makes
        n_big = 40
        prompts_big = [f"a photo of object number {i}" for i in range(n_big)]

        def sd_step_big():
            imgs = sd.generate_batch(prompts_big, list(range(n_big)), steps_sd, 7.5, 512, 512)
            return eng.encode_image(clip.preprocess_tensor(imgs), True)

        sd_step_big(); sync()
        sd_eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 1)
        eng.profile_begin()
        sd_step_big(); sync()
        prof_big = eng.profile_end()
        sd_eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 2)
        d_big, _ = timed(sd_step_big, 1, 1)
        gemm_tf_big = prof_big["gemm"]["work"] / (prof_big["gemm"]["ms"] * 1e-3) / 1e12 if prof_big["gemm"]["ms"] > 0 else 0.0
        # ---- BASELINE configs[4] end to end: the full three-method detector (text variants + SD references + consistency,
        # src/detector.py:345-439) on 4 queries x 3 generated references each, 20 steps -- generation dominates
        texts_sd, vocab_sd = make_captions(4)
        det = pkg.AdversarialDetector(pkg.DetectorConfig(clip_model=a.model, num_text_variants=N, num_reference_images=3),
                                      clip_model=clip, text_augmenter=WordReplaceVariants(N, vocab_sd),
                                      sd_generator=pkg.SDReferenceGenerator(
                                          pkg.SDReferenceConfig(num_images_per_prompt=3, num_inference_steps=steps_sd, use_text_variants=False,
                                                                filter_low_quality=False, enable_cache=False), sd_model=sd, clip_model=clip))
        d_full, res_full = timed(lambda: det.batch_detect(images[:4], texts_sd), 2, 1)
        assert len(res_full) == 4 and all("sd_reference" in r["detection_scores"] for r in res_full)
        # the same detector on 16 queries per call (48 generated references: the low-resolution UNet levels fill the chip)
        nq16 = min(16, B)
        texts_sd16, _ = make_captions(nq16, seed=5)
        d_full16, res16 = timed(lambda: det.batch_detect(images[:nq16], texts_sd16), 1, 1)
        assert len(res16) == nq16
        out["sd_reference"] = {"model": f"{sd.arch.name} geometry ({'v' if sd.arch.prediction_type == 'v_prediction' else 'epsilon'}-prediction, "
                                        f"heads {[sd.arch.heads_at(i) for i in range(len(sd.arch.block_out_channels))]}, cross-attention {sd.arch.cross_attention_dim}), random init",
                               "images_per_s": round(n_img * 2 / d_sd, 3), "images": n_img, "steps": steps_sd, "latent": "64x64",
                               "full_defense_qps": round(4 * 2 / d_full, 3),
                               "full_defense_qps_16_queries_per_call": round(nq16 / d_full16, 3),
                               "full_defense_note": "AdversarialDetector.batch_detect with all three methods (text_variants + sd_reference + "
                                                    "consistency), 4 queries x 3 references x 20 steps per batch (BASELINE configs[4])",
                               "seconds_per_batch": round(d_sd / 2, 3),
                               "streams": {"two_streams_images_per_s": round(n_img * 2 / d_sd, 3), "one_stream_images_per_s": round(n_img / d_sd1, 3),
                                           "note": "TVC_OPT_SD_STREAMS: the unconditional and the conditional half of every UNet evaluation on two "
                                                   "HIP streams (default) / on one; bit-identical images; kernel_ms_per_batch and gemm_tflops are "
                                                   "measured in the one-stream form (unoverlapped launch durations)"},
                               "batch_of_40": {"images_per_s": round(n_big / d_big, 3), "seconds_per_batch": round(d_big, 3),
                                               "gemm_tflops": round(gemm_tf_big, 1),
                                               "gemm_frac_of_peak": round(gemm_tf_big / PEAK_BF16_DENSE_TFLOPS, 4),
                                               "kernel_ms_per_batch": {c: round(v["ms"], 1) for c, v in prof_big.items()},
                                               "note": "same generator, 40 prompts x seeds per call (80 samples per UNet evaluation): the "
                                                       "low-resolution levels fill the 256 CUs; images bit-identical to the 12-image batch's"},
                               "unet_evaluations_per_batch": steps_sd + 1, "samples_per_evaluation": 2 * n_img,
                               "kernel_ms_per_batch": {c: round(v["ms"], 1) for c, v in prof.items()},
                               "gemm_tflops": round(gemm_tf, 1), "gemm_frac_of_peak": round(gemm_tf / PEAK_BF16_DENSE_TFLOPS, 4),
                               "gemm_tflop_per_image": round(prof["gemm"]["work"] / n_img / 1e12, 2),
                               "attention_tflops": round(prof["attention"]["work"] / (prof["attention"]["ms"] * 1e-3) / 1e12, 1) if prof["attention"]["ms"] > 0 else None,
                               "note": "random-init SD-1.5 geometry (no checkpoint without a network); UNet + VAE GEMMs through the tower "
                                       "GEMM kernel (3x3 convolutions as 9-plane GEMMs on a padded token layout, no im2col rows); "
                                       "attention = sd_flash_attention_kernel"}
        del sd

    if rank == 0 and not a.no_cpu_baseline and world == 1:
        nq = min(B, 64)
        cores = host_cpus()             # more threads than the cgroup quota only thrash
        bank_cpu = bank.float().cpu().numpy()
        img_c, tok_c = images[:nq].cpu(), tokens[:nq].cpu().long()
        oracle_scores = []
        v, done, secs = cpu_baseline(arch, weights, img_c, tok_c, bank_cpu, a.cpu_seconds, cores, scores_out=oracle_scores)
        if oracle_scores:
            # END-TO-END deviation of every tower mode's records from the fp32 CPU path, on the queries just timed
            cols = {"original_similarity": 0, "score_src": 5, "overall_exp": 10}
            devs = {}
            for mode, r_m in rec_modes.items():
                devs[mode] = {k: max(abs(float(r_m[i, c]) - o[k]) for i, o in enumerate(oracle_scores)) for k, c in cols.items()}
            if "parity_mode" in out:
                for mode in out["parity_mode"]:
                    out["parity_mode"][mode]["max_abs_score_dev"] = {k: float(f"{x:.3g}") for k, x in devs[mode].items()}
                out["parity_mode"]["bf16_default"] = {"max_abs_score_dev": {k: float(f"{x:.3g}") for k, x in devs["bf16"].items()}}
                out["parity_mode"]["note"] = (f"|record - fp32 CPU oracle| over the {len(oracle_scores)} queries of the cpu_baseline sample, "
                                              "END TO END (towers included); bar of BASELINE.json: 1e-4")
            else:
                out["score_dev_vs_cpu_oracle"] = {k: float(f"{x:.3g}") for k, x in devs["bf16"].items()}
        out["cpu_baseline"] = {"value": round(v, 3), "unit": "queries/s", "cores": cores, "kind": "port",
                               "sample": f"{done} queries of the same workload in {secs:.1f}s, oracle "
                                         f"(PyTorch-CPU fp32 towers + numpy scores), de-duplicated schedule"}
        out["speedup_vs_cpu"] = round(out["value"] / v, 1) if v > 0 else None
        if extras and "sd_reference" in out:
            # BASELINE configs[4]'s AUROC leg: the three-method defence (text variants + GENERATED references + consistency) on
            # PGD-perturbed inputs, HIP against the CPU oracle (oracle/defence_check.py: the checker, at a geometry the oracle
            # finishes in ~10 s; tests/test_gpu_auroc.py asserts the same check)
            from oracle import defence_check
            t_a = time.perf_counter()
            dc = defence_check.three_method_auroc(pkg, Q=128, N=4, J=2, steps=3)
            out["sd_reference"]["auroc_delta"] = round(dc["auroc_gpu"] - dc["auroc_oracle"], 5)
            out["sd_reference"]["auroc_check"] = {"auroc_gpu": round(dc["auroc_gpu"], 4), "auroc_oracle": round(dc["auroc_oracle"], 4),
                                                  "max_abs_aggregated_score_dev": float(f"{dc['max_abs_aggregated_dev']:.3g}"),
                                                  "queries": dc["Q"], "references_per_query": dc["references_per_query"],
                                                  "seconds": round(time.perf_counter() - t_a, 1),
                                                  "note": "toy CLIP + two-level latent-diffusion geometry, half the queries perturbed by the "
                                                          "in-tree PGDAttacker, references generated on both sides from the same prompts / seeds; "
                                                          "bar +-0.002 (the SD oracle is parity-unpinned)"}
        if extras:
            more = {}
            v2, d2, s2 = cpu_baseline(arch, weights, img_c, tok_c, bank_cpu, 12.0, cores, schedule="reference", max_queries=4)
            more["reference_schedule"] = {"value": round(v2, 4), "unit": "queries/s", "cores": cores, "kind": "port",
                                          "sample": f"{d2} queries in {s2:.1f}s, the reference's schedule (src/detector.py:461-471,573: "
                                                    f"N+2 image-tower passes and N+2 single-text passes per query)"}
            v3, d3, s3 = cpu_baseline(arch, weights, img_c, tok_c, bank_cpu, 10.0, 1, max_queries=2)
            more["one_thread"] = {"value": round(v3, 4), "unit": "queries/s", "cores": 1, "kind": "port",
                                  "sample": f"{d3} queries in {s3:.1f}s, de-duplicated schedule, torch.set_num_threads(1)"}
            # BASELINE configs[0] exactly: ViT-B/32, batch 8, N = 4, 1k-row bank, on the CPU
            a0 = pkg.get_arch("ViT-B/32")
            w0 = pkg.synth.make_clip_weights(a0, seed=0)
            i0 = pkg.synth.make_images(8, a0.image_size, seed=1)
            t0 = pkg.synth.make_tokens(8, 4, a0.ctx, seed=2).long()
            b0 = pkg.synth.make_bank(1000, a0.embed_dim, seed=7).numpy()
            v4, d4, s4 = cpu_baseline(a0, w0, i0, t0, b0, 10.0, cores)
            more["configs0_vit_b32_b8_n4_r1k"] = {"value": round(v4, 3), "unit": "queries/s", "cores": cores, "kind": "port",
                                                   "sample": f"{d4} queries in {s4:.1f}s, de-duplicated schedule (BASELINE configs[0])"}
            out["cpu_baselines_extra"] = more
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1 or a.shard_bank:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
