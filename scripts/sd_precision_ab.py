"""A/B of the latent-diffusion model's 16-bit format (TVC_OPT_SD_PRECISION: bf16 / fp16): images/s of one batched generation
(12 images x 20 steps at SD-1.5 geometry, 64 x 64 latents + VAE decode, seeded random weights), unprofiled, both modes in ONE
process, alternating, three repeats each; prints every run, then each mode's median and spread (min .. max), then each mode's
per-category kernel times of one-stream generations (where a difference between the modes sits).
Usage: python scripts/sd_precision_ab.py [steps] [n] [modes, e.g. bf16 or bf16,fp16] [repeats]
(one mode alone, e.g. `20 12 bf16`, is the leg to run on an older build for comparison)."""
import hashlib, importlib, json, os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("multimodal-detection-consistency_amd")
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
modes = sys.argv[3].split(",") if len(sys.argv) > 3 else ["bf16", "fp16"]
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 3
models = {}
for m in modes:          # one model (own engine, own weights copy) per mode; a build without the option only knows bf16
    cfg = pkg.SDModelConfig(random_init=True, precision=m) if m != "bf16" else pkg.SDModelConfig(random_init=True)
    models[m] = pkg.StableDiffusionModel(cfg)
prompts = [f"a photo of object number {i}" for i in range(n)]
rates = {m: [] for m in modes}
for m in modes:
    models[m].generate_batch(prompts, list(range(n)), 2, 7.5, 512, 512)          # warm-up (workspaces)
for rep in range(repeats):
    for m in modes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        imgs = models[m].generate_batch(prompts, list(range(n)), steps, 7.5, 512, 512)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates[m].append(n / dt)
        md5 = hashlib.md5(torch.as_tensor(imgs).float().cpu().numpy().tobytes()).hexdigest()
        print(json.dumps({"precision": m, "repeat": rep, "images": n, "steps": steps, "seconds": round(dt, 4),
                          "images_per_s": round(n / dt, 3), "finite": bool(torch.isfinite(imgs).all()), "images_md5": md5}), flush=True)
for m in modes:
    r = rates[m]
    print(json.dumps({"precision": m, "images_per_s_median": round(statistics.median(r), 3), "min": round(min(r), 3),
                      "max": round(max(r), 3), "spread": round(max(r) - min(r), 3)}), flush=True)
# where a difference sits: the in-process category times (HIP events around every launch) of one more generation per mode, in the
# one-stream form so that launches do not overlap; alternating, `repeats` times, medians
prof = {m: {} for m in modes}
for rep in range(repeats):
    for m in modes:
        eng = models[m].text_engine
        eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 1)
        try:
            models[m].generate_batch(prompts, list(range(n)), 2, 7.5, 512, 512)          # the one-stream workspaces
            torch.cuda.synchronize()
            eng.profile_begin()
            models[m].generate_batch(prompts, list(range(n)), steps, 7.5, 512, 512)
            torch.cuda.synchronize()
            p = eng.profile_end()
        finally:
            eng.set_option(pkg._lib.TVC_OPT_SD_STREAMS, 2)
        for c, v in p.items():
            prof[m].setdefault(c, []).append(v["ms"])
for m in modes:
    print(json.dumps({"precision": m, "one_stream_category_ms_median": {c: round(statistics.median(v), 2) for c, v in prof[m].items()},
                      "launches": {c: int(p[c]["launches"]) for c in p}}), flush=True)
