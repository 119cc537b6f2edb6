"""Bit-identity of two builds of libtvc_hip.so (a refactor against its parent commit):

    python scripts/lib_ab.py OLD.so NEW.so [--timeout 240] [--keep DIR] [--only attention|bank|cluster|sd|slot]

One fresh child process per library (selected with TVC_LIB_PATH, each child under its own ``timeout -k 10``; the second starts
only if the first exited 0).  A child runs seed-fixed inputs through the library and writes one .npy file per result; the
parent compares the two sets byte for byte and prints one line per array and one JSON summary line.  Exit status 0 = every
array identical.

Covered: the towers at the toy CLIP geometry of the GPU tests with seeded random weights -- encode_image (B = 3), encode_text
with group = 3 over 6 texts of different lengths (packing and prefix sharing on), encode_text_hidden -- in all four
precisions, each with TVC_OPT_POOLED_LAST_LAYER on and off; the gradient path (encode_image_grad + encode_image_backward,
B = 2); the kernel entries layernorm, layernorm_f16 and layernorm_backward (with and without dres) on the piece-loop edge
shapes; one latent-diffusion transformer block and one resnet block at 8 x 8 (ln_bf16_kernel with and without `add`, GEGLU,
the adds); the bank search (bank_cases below: every filter kernel, both tau kernels, the select, the dense fallback and the
shard merge; the children inherit TVC_BANK_RING / TVC_BANK_SKINNY / TVC_BANK_SKINNY_SAMPLE, so a run with all three at 0
reaches bank_search_kernel<true> and the dense sample for small M); k-means on a bank slot and the IVF search (cluster_cases
below: assign and update with an empty cluster and an out-of-range label, the probe, the scan with padding and with the select's
LDS and global-memory paths); the other tile passes over a slot (slot_cases below: the closest pair over three row tiles and
over a single row, the radius graph at its median distance, the retrieval ranks' two tile passes and metrics, each on a bf16
and an fp32 slot); the latent-diffusion generator end to end (sd_cases below: the UNet at two sizes, the VAE decode,
the sampling loop on two streams and on one, chunked, and with v-prediction, all six block kinds, in bf16 and in fp16); the
five swapped-MFMA attention kernels at every instantiation their launchers can pick (attention_cases below: attention_ex in bf16 and fp16 -- <17, EXACT>, <4, EXACT>, <2>, <6>, <18>, <4, WPS 2>, the causal
<2>, <6>, <18> on packed rows with and without shared prefixes, both pooled forms --, attention_split_ex's six, attention_backward
at T = 257, 50, 100 and 1, the streaming kernel at every head dim and workgroup shape in both SD precisions and with separate
strides).  --only NAME runs one of the *_cases functions alone.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
LN_SHAPES = ((1, 64), (5, 260), (7, 1024))
TEXT_LENS = (19, 12, 9, 17, 15, 5)      # ids between SOT and EOT of the 6 texts


def bank_cases(pkg, save) -> None:
    """topk_idx, topk_sim and (where requested) the moments of seeded searches; bank.hip names the kernels."""
    import ctypes as C
    import torch
    L = pkg._lib

    def unit(shape, seed):
        return torch.nn.functional.normalize(torch.randn(shape, generator=torch.Generator().manual_seed(seed)), dim=-1)

    eng = pkg.TVCEngine()

    def search(tag, q, k, **kw):
        idx, sim, mom = eng.bank_search(q, k, **kw)
        eng.bank_status()
        save(f"bank_{tag}_idx", idx)
        save(f"bank_{tag}_sim", sim)
        if mom is not None:
            save(f"bank_{tag}_mom", mom)

    # skinny filter + skinny sample + kth_groups_kernel
    eng.set_bank(unit((1000, 512), 11).to(torch.bfloat16).cuda())
    search("1000x48", unit((48, 512), 12).cuda(), 5, want_moments=False)
    # skinny filter over two planes + the dense sample + kth_bound_kernel
    eng.set_bank(unit((4097, 128), 13).cuda())
    search("4097x17", unit((17, 128), 14).cuda(), 7, want_moments=False)
    # the 256-query-tile kernels in the blocked item order: all products (moments), the ring filter, the filter switched off
    q770 = unit((770, 64), 15).cuda()
    for R, dt, seed in ((4000, torch.float32, 16), (90001, torch.bfloat16, 17)):
        eng.set_bank(unit((R, 64), seed).to(dt).cuda())
        search(f"{R}x770_mom", q770, 5, count_thr=0.05)
        search(f"{R}x770_filter", q770, 5, want_moments=False)
        eng.set_option(L.TVC_OPT_BANK_FILTER, 0)
        search(f"{R}x770_nofilter", q770, 5, want_moments=False)
        eng.set_option(L.TVC_OPT_BANK_FILTER, 1)
        if R == 4000:
            search("4000x770_offset", q770, 5, idx_offset=123456, want_moments=False)
            # row_topk_kernel with moments: the dense fallback on 70 query rows
            q = q770[:70].contiguous()
            i2 = torch.empty((70, 5), dtype=torch.int32, device="cuda:0")
            s2 = torch.empty((70, 5), dtype=torch.float32, device="cuda:0")
            m2 = torch.empty((70, 4), dtype=torch.float32, device="cuda:0")
            rc = eng.lib.tvc_bank_search_dense(eng.handle, C.c_void_p(q.data_ptr()), 70, 5, 0.05, 0, C.c_void_p(i2.data_ptr()),
                                               C.c_void_p(s2.data_ptr()), C.c_void_p(m2.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            save("bank_dense_idx", i2)
            save("bank_dense_sim", s2)
            save("bank_dense_mom", m2)
    # row_topk_kernel where its order and admission rule decide (tests/test_gpu_path.py::test_bank_search_dense_degenerate_rows):
    # a row stored three times, 10 rows of zeros, a zero query, k = 128 over 100 rows of which one is all NaN
    rows = unit((100, 128), 51)
    rows[60] = rows[93] = rows[17]
    rows[70:80] = 0.0
    q = unit((5, 128), 52)
    q[1] = 0.0
    q = q.cuda()
    for tag, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        for nan in (True, False):                 # moments only over the NaN-free bank
            b = rows.to(dt)
            if nan:
                b[41] = float("nan")
            eng.set_bank(b.cuda())
            i2 = torch.empty((5, 128), dtype=torch.int32, device="cuda:0")
            s2 = torch.empty((5, 128), dtype=torch.float32, device="cuda:0")
            m2 = None if nan else torch.empty((5, 4), dtype=torch.float32, device="cuda:0")
            rc = eng.lib.tvc_bank_search_dense(eng.handle, C.c_void_p(q.data_ptr()), 5, 128, 0.05, 0, C.c_void_p(i2.data_ptr()),
                                               C.c_void_p(s2.data_ptr()), None if nan else C.c_void_p(m2.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            save(f"bank_dense_short_{tag}_nan{int(nan)}_idx", i2)
            save(f"bank_dense_short_{tag}_nan{int(nan)}_sim", s2)
            if m2 is not None:
                save(f"bank_dense_short_{tag}_mom", m2)
    # topk_merge_kernel on the inputs of tests/test_gpu_api.py::test_topk_merge_kernel
    W, M, k, kf, D = 4, 37, 8, 3, 128
    g = torch.Generator().manual_seed(0)
    sim = torch.rand((W, M, k), generator=g).sort(dim=-1, descending=True).values
    idx = torch.stack([torch.randperm(1000, generator=g)[:k] + 1000 * w for w in range(W) for _ in range(M)]).view(W, M, k).int()
    idx[3, :, 5:] = -1
    feat = torch.randn((W, M, kf, D), generator=g)
    mom = torch.rand((W, M, 4), generator=g)
    for name, t in zip(("idx", "sim", "feat", "mom"), eng.topk_merge(idx.cuda(), sim.cuda(), feat.cuda(), mom.cuda())):
        save(f"merge_{name}", t)
    torch.cuda.synchronize()
    eng.close()


def cluster_cases(pkg, save) -> None:
    """k-means assign and update on a bf16 and an fp32 slot, the IVF probe, and IVF scans over hand-made lists (kmeans.hip and
    ivf.hip name the kernels); the entries and call forms of tests/test_gpu_kmeans.py and tests/test_gpu_ivf.py."""
    import numpy as np
    import torch
    eng = pkg.TVCEngine()
    dev = eng.device

    def unit(shape, seed):
        return torch.nn.functional.normalize(torch.randn(shape, generator=torch.Generator().manual_seed(seed)), dim=-1)

    R, K, D = 1000, 37, 128
    X, cent = unit((R, D), 21), (unit((K, D), 22) * 0.9).to(dev)
    for tag, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        eng.set_bank(X.to(dt).to(dev), name="ab")
        labels, score, dist2 = eng.kmeans_assign(cent, bank="ab")
        lab = labels.clone()
        lab[lab == 5] = 6                         # cluster 5 stays empty
        lab[3] = K + 9                            # a label outside [0, K)
        out = eng.kmeans_update(lab, cent, bank="ab", want_lists=True)
        for name, t in zip(("labels", "score", "dist2", "centroids", "counts", "offsets", "order"), (labels, score, dist2) + tuple(out)):
            save(f"km_{tag}_{name}", t)
    M, nlist, nprobe, k = 9, 300, 8, 10
    Q = unit((M, D), 23).to(dev)
    C = unit((nlist, D), 24) * 0.8
    lists, score = eng.ivf_probe(Q, C.to(dev), nprobe)
    save("ivf_probe_lists", lists)
    save("ivf_probe_score", score)
    # lists of 0 .. 20 rows, original ids shuffled (ascending inside a list)
    rng = np.random.default_rng(25)
    lengths = rng.integers(0, 21, nlist)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    rows = int(offsets[-1])
    ids = rng.permutation(rows)
    for l in range(nlist):
        ids[offsets[l]:offsets[l + 1]].sort()
    probes = np.stack([rng.choice(nlist, nprobe, replace=False) for _ in range(M)])
    probes[2, 5] = -1
    probes[4, 3] = probes[4, 0]                   # a list probed twice
    short = probes.copy()
    short[:, 1:] = -1                             # one list of at most 20 rows per query: most have fewer than k, the rest is padding
    Xs = unit((rows, D), 26)
    for tag, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        eng.set_bank(Xs.to(dt).to(dev), name="ab")
        # 4097 declared rows: nprobe x pitch floats no longer fit the select's LDS (plan.select_lds == 0)
        for case, p, max_rows in (("lds", probes, 20), ("pad", short, 20), ("nolds", probes, 4097)):
            ix = pkg.IVFIndex(name="ab", nlist=nlist, centroids=C.to(dev), offsets=torch.from_numpy(offsets.astype(np.int32)).to(dev),
                              ids=torch.from_numpy(ids.astype(np.int32)).to(dev), max_list_rows=max_rows, rows=rows, dim=D)
            got = eng.ivf_scan(Q, k, torch.from_numpy(p.astype(np.int32)).to(dev), ix, idx_offset=1000)
            eng.bank_status()
            for name, t in zip(("idx", "sim", "pos"), got):
                save(f"ivf_scan_{tag}_{case}_{name}", t)
    torch.cuda.synchronize()
    eng.close()


def slot_cases(pkg, save) -> None:
    """The GEMM-tile passes over a bank slot that cluster_cases does not reach, on a bf16 and an fp32 slot: the closest pair
    (nearest.hip) at R = 700 -- three row tiles: diagonal tiles, off-diagonal tiles and padding -- and at R = 1; the radius graph
    (dbscan.hip) at R = 513 with eps = the median pairwise distance of the rows, so about half the bits are set; the retrieval
    ranks (rank.hip: both tile passes and the metrics) of 300 queries over 1000 rows under 20 labels."""
    import torch
    eng = pkg.TVCEngine()
    dev = eng.device

    def unit(shape, seed):
        return torch.nn.functional.normalize(torch.randn(shape, generator=torch.Generator().manual_seed(seed)), dim=-1)

    D = 128
    X700, X513, X1000, Q = unit((700, D), 61), unit((513, D), 62), unit((1000, D), 63), unit((300, D), 64).to(dev)
    i, j = torch.triu_indices(513, 513, offset=1)
    eps = float(torch.cdist(X513.double(), X513.double())[i, j].median())
    g = torch.Generator().manual_seed(65)
    qlabels, glabels = torch.randint(0, 20, (300,), generator=g), torch.randint(0, 20, (1000,), generator=g)
    for tag, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        for R in (700, 1):
            eng.set_bank(X700[:R].to(dt).to(dev), name="ab")
            for name, t in zip(("pair", "pair_sim", "partner", "sim"), eng.closest_pair(bank="ab")):
                save(f"nn_{tag}_{R}_{name}", t)
        eng.set_bank(X513.to(dt).to(dev), name="ab")
        adj, degree = eng.radius_graph(eps, bank="ab")
        save(f"radius_{tag}_adj", adj)
        save(f"radius_{tag}_degree", degree)
        eng.set_bank(X1000.to(dt).to(dev), name="ab")
        rk = eng.retrieval_ranks(Q, qlabels, glabels, bank="ab")
        for name in ("tgt_off", "tgt_row", "tgt_sim", "pos", "hist", "ap", "rr", "hits", "dcg", "idcg"):
            save(f"rank_{tag}_{name}", getattr(rk, name))
    torch.cuda.synchronize()
    eng.close()


def sd_cases(pkg, save) -> None:
    """Every latent-diffusion entry point that runs the model's host code (csrc/tvc_sd.cpp) at the toy geometry, in both 16-bit
    formats: tvc_sd_unet (n = 2 at 16 x 16, n = 3 at 8 x 24), tvc_sd_vae_decode (n = 3), tvc_sd_generate of 6 steps with
    TVC_OPT_SD_STREAMS 2 and 1, once in chunks (3 images at 96 x 96 latents under TVC_OPT_SD_ARENA_BYTES = 1 << 28, the option's
    minimum: a pair needs over 100 MB there, so the images run as 2 + 1), 4 steps of a v-prediction model, and the six kinds of
    tvc_sd_block."""
    import dataclasses
    import torch
    L = pkg._lib
    arch = pkg.SDArch(block_out_channels=(64, 128), down_block_attn=(True, False), layers_per_block=1, heads=8,
                      cross_attention_dim=128, vae_block_out_channels=(64, 128), vae_layers_per_block=1, sample_size=16)
    uw, vw = pkg.make_sd_weights(arch, seed=3)
    g = torch.Generator().manual_seed(31)
    lat = torch.randn((3, 4, 16, 16), generator=g)
    lat_wide = torch.randn((3, 4, 8, 24), generator=g)
    lat96 = torch.randn((3, 4, 96, 96), generator=g)
    cond, uncond = torch.randn((3, arch.ctx, 128), generator=g), torch.randn((3, arch.ctx, 128), generator=g)
    x64, x128, x256 = (torch.randn((2, c, hw, hw), generator=g) for c, hw in ((64, 16), (128, 8), (256, 8)))
    temb = torch.randn((2, arch.time_dim), generator=g)
    for prec in ("bf16", "fp16"):
        eng = pkg.TVCEngine()
        k = pkg.SDKernels(eng, arch, uw, vw, precision=prec)
        save(f"sd_{prec}_unet_2x16x16", k.unet(lat[:2], 951.0, cond[:2]))
        save(f"sd_{prec}_unet_3x8x24", k.unet(lat_wide, 1.0, cond))
        save(f"sd_{prec}_vae_3", k.vae_decode(lat))
        for streams in (2, 1):
            eng.set_option(L.TVC_OPT_SD_STREAMS, streams)
            out, img = k.generate(cond, uncond, lat, 6, 7.5)
            save(f"sd_{prec}_gen6_streams{streams}_lat", out)
            save(f"sd_{prec}_gen6_streams{streams}_img", img)
        eng.set_option(L.TVC_OPT_SD_STREAMS, 2)
        eng.set_option(L.TVC_OPT_SD_ARENA_BYTES, 1 << 28)
        save(f"sd_{prec}_gen6_chunked_lat", k.generate(cond, uncond, lat96, 6, 7.5, decode=False)[0])
        eng.set_option(L.TVC_OPT_SD_ARENA_BYTES, 48 << 30)
        blocks = ((0, "down_blocks.0.resnets.0.", x64, 64, dict(temb=temb)), (0, "up_blocks.0.resnets.0.", x256, 128, dict(temb=temb)),
                  (1, "down_blocks.0.attentions.0.", x64, 64, dict(ctx=cond[:2])),
                  (2, "decoder.mid_block.attentions.0.", x128, 128, dict(vae=True)),
                  (3, "down_blocks.0.resnets.0.conv1.", x64, 64, {}), (4, "down_blocks.0.downsamplers.0.conv.", x64, 64, {}),
                  (5, "up_blocks.0.upsamplers.0.conv.", x128, 128, {}))
        for j, (kind, prefix, x, cout, kw) in enumerate(blocks):
            save(f"sd_{prec}_block{j}_kind{kind}", k.block(kind, prefix, x, cout, **kw))
        kv = pkg.SDKernels(eng, dataclasses.replace(arch, prediction_type="v_prediction"), uw, vw, precision=prec)
        save(f"sd_{prec}_gen4_vpred_lat", kv.generate(cond[:2], uncond[:2], lat[:2], 4, 7.5, decode=False)[0])
        torch.cuda.synchronize()
        eng.close()


def attention_cases(pkg, save) -> None:
    """The five swapped-MFMA attention kernels (csrc/attn_frag.hpp) through their own entry points on seeded random rows, at
    the smallest shape that selects each instantiation a launcher can pick: attention_ex in bf16 and fp16 (<17, EXACT>,
    <4, EXACT>, <2>, <6>, <18>, <4, WPS 2> non-causal; causal <2>, <6>, <18> on packed rows, plain and with shared prefixes;
    both pooled forms), attention_split_ex (<2 | 6 | 18, causal | not>, dense, packed, with prefixes), attention_backward
    (T = 257, 50, 100, 1) and the streaming kernel (every head dim at workgroup shape 1, head dims <= 80 at shapes 2 and 3,
    both SD precisions, separate strides)."""
    import torch
    eng = pkg.TVCEngine()
    dev = eng.device
    pool = torch.randn(3 * 32 * 257 * 8 * 80, generator=torch.Generator().manual_seed(41)).to(dev)

    def rows(n, width, dt, skip=0):                       # [n, width] of the seeded pool, from element `skip` on
        return pool[skip:skip + n * width].view(n, width).to(dt).contiguous()

    def i32(v):
        return None if v is None else torch.tensor(v, dtype=torch.int32, device=dev)

    def packed(lens, prefix=None):                        # starts, and pfx from (P, base sequence) pairs
        st = [0]
        for n in lens:
            st.append(st[-1] + n)
        return st, None if prefix is None else [P for P, _ in prefix] + [st[b] for _, b in prefix]

    # own rows per sequence: lengths that straddle a 16-row tile; (P, base): P rows of the base sequence's are shared
    CAUSAL = {20: ((15, 16, 17, 20), (17, 5, 1, 16), ((0, 0), (15, 0), (16, 0), (0, 3))),
              77: ((33, 77, 16, 15), (33, 44, 15, 16), ((0, 0), (33, 0), (17, 0), (0, 3))),
              200: ((200, 17, 129), (100, 100, 33, 17), ((0, 0), (100, 0), (15, 0), (0, 3)))}
    heads = 3
    for f16 in (False, True):
        dt, tag = (torch.float16, "att_f16") if f16 else (torch.bfloat16, "att_bf16")

        def ex(name, n_seq, seq_len, causal, lens=None, prefix=None, n_rows=None, **kw):
            st, pf = packed(lens, prefix) if lens is not None else (None, None)
            n_rows = n_rows if n_rows is not None else (st[-1] if st else n_seq * seq_len)
            out = torch.zeros((n_seq if kw.get("pool_mode") else n_rows, heads * 64), dtype=dt, device=dev)
            save(f"{tag}_{name}", eng.attention_ex(rows(n_rows, 3 * heads * 64, dt), n_seq, seq_len, heads, causal, starts=i32(st),
                                                   pfx=i32(pf), f16=f16, out=out, **kw))

        for T in (257, 50, 20, 90, 200):
            ex(f"full_dense_{T}", 2, T, False)
        ex("full_packed_50", 4, 50, False, lens=(15, 16, 17, 33))
        for T, (plain, own, prefix) in CAUSAL.items():
            ex(f"causal_packed_{T}", len(plain), T, True, lens=plain)
            ex(f"causal_prefix_{T}", len(own), T, True, lens=own, prefix=prefix)
        ex("pool1_full_dense_257", 2, 257, False, pool_mode=1)
        ex("pool1_causal_packed_77", 4, 77, True, lens=CAUSAL[77][0], pool_mode=1)
        ex("pool2_causal_packed_77", 4, 77, True, lens=CAUSAL[77][0], pool_mode=2)
        ex("pool2_causal_prefix_20", 4, 20, True, lens=CAUSAL[20][1], prefix=CAUSAL[20][2], pool_mode=2)
        ex("pool2_causal_dense_77", 3, 77, True, pool_mode=2, pool_row=i32((76, 77 + 16, 2 * 77 + 15)))
        ex("pool2_full_dense_50", 3, 50, False, pool_mode=2, pool_row=i32((49, 50 + 17, 100)))

    def split(name, n_seq, seq_len, causal, lens=None, prefix=None):
        st, pf = packed(lens, prefix) if lens is not None else (None, None)
        n_rows = st[-1] if st else n_seq * seq_len
        save(f"att_split_{name}", eng.attention_split_ex(rows(n_rows, 3 * heads * 64, torch.float32), n_seq, seq_len, heads, causal,
                                                         starts=i32(st), pfx=i32(pf)))

    for T, (plain, own, prefix) in CAUSAL.items():
        split(f"full_dense_{T}", 2, T, False)
        split(f"full_packed_{T}", len(plain), T, False, lens=plain)
        split(f"causal_dense_{T}", 2, T, True)
        split(f"causal_packed_{T}", len(plain), T, True, lens=plain)
        split(f"causal_prefix_{T}", len(own), T, True, lens=own, prefix=prefix)

    for T in (257, 50, 100, 1):
        qkv, dout = rows(2 * T, 3 * 2 * 64, torch.bfloat16), rows(2 * T, 2 * 64, torch.bfloat16, skip=2 * T * 3 * 2 * 64)
        save(f"att_bwd_{T}", eng.attention_backward(qkv, dout, 2, T, 2))

    sa = pkg.sd_model.streaming_attention
    DIMS = (8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 128, 160)
    for prec, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        eng.set_sd_precision(prec)

        def sd(name, n, hd, dh, Tq, Tk, pad=None):
            C, (pq, pk, pv, po) = hd * dh, pad or (0, 0, 0, 0)
            q, k = rows(n * Tq, C + pq, dt), rows(n * Tk, C + pk, dt, skip=n * Tq * (C + pq))
            v = rows(n * Tk, C + pv, dt, skip=n * Tq * (C + pq) + n * Tk * (C + pk))
            out = sa(eng, q, k, v, n, hd, ld=(C + pq, C + pk, C + pv, C + po), dh=dh) if pad else sa(eng, q, k, v, n, hd)
            save(f"att_sd_{prec}_{name}_dh{dh}_{Tq}x{Tk}", out)

        for j, dh in enumerate(DIMS):
            sd("shape1", 2, 3, dh, (65, 130, 257)[j % 3], (77, 130)[j % 2])          # 6 items: 4 waves x 1 block
            if dh <= 80:                                  # 256 items: 4 waves x 2 blocks at Tq = 130, 8 waves x 2 blocks at 257
                sd("shape2", 32, 8, dh, 130, (130, 77)[j % 2])
                sd("shape3", 32, 8, dh, 257, (77, 130)[j % 2])
        for name, n, hd, Tq in (("strides1", 2, 3, 65), ("strides2", 32, 8, 130), ("strides3", 32, 8, 257)):
            sd(name, n, hd, 40, Tq, 130, pad=(8, 16, 24, 4))
    eng.set_sd_precision("bf16")
    torch.cuda.synchronize()
    eng.close()


def child(out_dir: Path, only: str = "") -> None:
    import torch
    sys.path.insert(0, str(ROOT))
    pkg = importlib.import_module("multimodal-detection-consistency_amd")
    L = pkg._lib

    def save(name: str, t) -> None:
        t = t.detach().cpu().contiguous()
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.view(torch.int16)
        np.save(out_dir / (name + ".npy"), t.numpy())

    if only:
        {"attention": attention_cases, "bank": bank_cases, "cluster": cluster_cases, "sd": sd_cases, "slot": slot_cases}[only](pkg, save)
        return

    arch = pkg.get_arch("ViT-T/16-test")
    vw, tw = pkg.synth.make_clip_weights(arch, seed=0)
    eng = pkg.TVCEngine(arch, vw, tw)
    imgs = pkg.synth.make_images(3, arch.image_size, seed=1).cuda()
    # 2 groups of (original, 2 variants), each text cut to a length of its own
    toks = pkg.synth.make_tokens(2, 2, arch.ctx, seed=2, min_len=TEXT_LENS[0], max_len=TEXT_LENS[0]).view(-1, arch.ctx)
    for j, n in enumerate(TEXT_LENS):
        toks[j, 1 + n] = pkg.synth.EOT
        toks[j, 2 + n:] = 0
    toks = toks.cuda()
    for prec in ("bf16", "fp16", "split", "fp32"):
        eng.set_precision(prec)
        for pooled in (1, 0):
            eng.set_option(L.TVC_OPT_POOLED_LAST_LAYER, pooled)
            tag = f"{prec}_pooled{pooled}"
            save(f"image_{tag}", eng.encode_image(imgs))
            save(f"text_{tag}", eng.encode_text(toks, group=3))
            save(f"hidden_{tag}", eng.encode_text_hidden(toks))
    eng.set_precision("bf16")
    eng.set_option(L.TVC_OPT_POOLED_LAST_LAYER, 1)
    g = torch.Generator().manual_seed(3)
    px = imgs[:2].contiguous()
    save("grad_fwd", eng.encode_image_grad(px))
    save("grad_bwd", eng.encode_image_backward(torch.randn((2, arch.embed_dim), generator=g).cuda()))
    for rows, d in LN_SHAPES:
        x = (torch.randn((rows, d), generator=g) * 3 + 1).cuda()
        gam, bet = torch.randn(d, generator=g).cuda(), torch.randn(d, generator=g).cuda()
        dy = torch.randn((rows, d), generator=g).to(torch.bfloat16).cuda()
        dres = torch.randn((rows, d), generator=g).cuda()
        save(f"ln_{rows}x{d}", eng.layernorm(x, gam, bet))
        save(f"ln_f16_{rows}x{d}", eng.layernorm_f16(x, gam, bet))
        save(f"ln_bwd_{rows}x{d}", eng.layernorm_backward(x, dy, gam, None))
        save(f"ln_bwd_dres_{rows}x{d}", eng.layernorm_backward(x, dy, gam, dres))
    eng.close()

    sarch = pkg.SDArch(block_out_channels=(64, 128), down_block_attn=(True, False), layers_per_block=1, heads=8,
                       cross_attention_dim=128, vae_block_out_channels=(64, 128), vae_layers_per_block=1, sample_size=16)
    uw, _ = pkg.make_sd_weights(sarch, seed=3, which="unet")
    eng = pkg.TVCEngine()
    k = pkg.SDKernels(eng, sarch, uw, None)
    x = torch.randn((2, 64, 8, 8), generator=g)
    ctx = torch.randn((2, sarch.ctx, sarch.cross_attention_dim), generator=g)
    temb = torch.randn((2, sarch.time_dim), generator=g)
    save("sd_transformer", k.block(1, "down_blocks.0.attentions.0.", x, 64, ctx=ctx))
    save("sd_resnet", k.block(0, "down_blocks.0.resnets.0.", x, 64, temb=temb))
    torch.cuda.synchronize()
    eng.close()
    bank_cases(pkg, save)
    cluster_cases(pkg, save)
    slot_cases(pkg, save)
    sd_cases(pkg, save)
    attention_cases(pkg, save)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--keep", default=None, help="directory that keeps the .npy files (default: a temporary one)")
    ap.add_argument("--only", default="", choices=("", "attention", "bank", "cluster", "sd", "slot"), help="one *_cases function alone")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(Path(a.child), a.only)
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(a.keep) if a.keep else Path(tmp)
        dirs = []
        for tag, lib in (("old", a.old), ("new", a.new)):
            d = base / tag
            d.mkdir(parents=True, exist_ok=True)
            dirs.append(d)
            env = dict(os.environ, TVC_LIB_PATH=str(Path(lib).resolve()))
            rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, __file__, a.old, a.new, "--child", str(d), "--only", a.only],
                                env=env).returncode
            if rc != 0:
                print(json.dumps({"lib_ab": "child failed", "library": lib, "exit": rc}), flush=True)
                return 2
        names = sorted(p.name for p in dirs[0].glob("*.npy"))
        missing = sorted(set(names) ^ {p.name for p in dirs[1].glob("*.npy")})
        differ = []
        for n in names:
            if n in missing:
                continue
            same = (dirs[0] / n).read_bytes() == (dirs[1] / n).read_bytes()
            line = f"{n[:-4]:28s} {'identical' if same else 'DIFFERS'}"
            if not same:
                o, w = np.load(dirs[0] / n), np.load(dirs[1] / n)
                line += f"  {int((o != w).sum())} of {o.size} elements"
                differ.append(n[:-4])
            print(line)
        ok = bool(names) and not differ and not missing
        print(json.dumps({"lib_ab": "identical" if ok else "DIFFERENT", "arrays": len(names), "differ": differ, "missing": missing}),
              flush=True)
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
