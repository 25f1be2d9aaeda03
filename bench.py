#!/usr/bin/env python3
"""Flagship benchmark: TIGER training step on Amazon-Beauty-shaped synthetic
data (BASELINE.json: "Recall@10 + train samples/sec, TIGER Amazon-Beauty at
1/2/4/8 MI355X").

Measures whole-job train samples/sec for the reference's shipped TIGER
config (config/tiger/amazon/tiger.gin: d_model 128 -> attn 384, 6 heads,
4+4 layers, sem_id_dim 3, codebook 256, batch 256/GPU, 20-item histories =
61 encoder tokens), bf16 autocast, full fwd+bwd+clip+AdamW step per
iteration, DDP over RCCL/xGMI for N>1 (weak scaling: per-GPU batch fixed).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W]
                       [--dump-outputs DIR] [--full]
For N>1 the driver launches via torch.distributed.run with one rank per GPU.

A plain run sets up, warms up, times exactly --steps steps and prints the
result line. --dump-outputs DIR additionally writes what the last timed
step produced (loss, gradients, updated fp32 parameters) as DIR/<name>.npy
so two builds can be compared output for output. On the GPU that step
starts from the model/optimizer/RNG state reached after the --warmup steps
(restored with the clock stopped): the inputs, the initial weights and
that state depend only on the arguments, while a state reached through
hundreds of training steps would not be repeatable beyond rounding.
--full is reserved for measurements beyond the headline figure; the
flagship benchmark has none, so it changes nothing.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch


def build_batch(batch_size: int, n_items: int, sem_id_dim: int,
                codebook_size: int, num_users: int, device, seed: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    L = n_items * sem_id_dim
    item_ids = torch.randint(0, codebook_size, (batch_size, L), generator=g)
    ttype = (torch.arange(L) % sem_id_dim).unsqueeze(0).expand(batch_size, -1)
    tgt = torch.randint(0, codebook_size, (batch_size, sem_id_dim), generator=g)
    tgt_type = torch.arange(sem_id_dim).unsqueeze(0).expand(batch_size, -1)
    user = torch.randint(0, num_users, (batch_size, 1), generator=g)
    # realistic ragged histories: ~30% of rows left-padded shorter
    mask = torch.ones(batch_size, L, dtype=torch.long)
    lens = torch.randint(5, n_items + 1, (batch_size,), generator=g)
    for i in range(0, batch_size, 3):
        mask[i, lens[i] * sem_id_dim:] = 0
    return {
        "user_input_ids": user.to(device),
        "item_input_ids": item_ids.to(device),
        "token_type_ids": ttype.contiguous().to(device),
        "target_input_ids": tgt.to(device),
        "target_token_type_ids": tgt_type.contiguous().to(device),
        "seq_mask": mask.to(device),
    }


def _enable_tuned_gemms() -> None:
    """Load the pre-tuned hipBLASLt solution table (benchmarks/tunableop0.csv,
    produced once with PYTORCH_TUNABLEOP_TUNING=1 on an MI355X)."""
    repo = os.path.dirname(os.path.abspath(__file__))
    csv = os.path.join(repo, "benchmarks", "tunableop.csv")
    if os.path.exists(os.path.join(repo, "benchmarks", "tunableop0.csv")) \
            and os.environ.get("PYTORCH_TUNABLEOP_TUNING", "0") != "1":
        os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "0")
        os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", csv)


# --dump-outputs: at most this many elements per array (3 arrays of fp32
# => <= 48 MB in all); larger arrays are cut to a fixed seeded sample.
_DUMP_MAX_ELEMS = 4 * 1024 * 1024


def _dump_array(path: str, t: torch.Tensor) -> None:
    import numpy as np

    a = t.detach().reshape(-1).float().cpu().numpy()
    if a.size > _DUMP_MAX_ELEMS:
        idx = np.random.default_rng(0).choice(a.size, _DUMP_MAX_ELEMS,
                                              replace=False)
        a = a[np.sort(idx)]
    np.save(path, np.ascontiguousarray(a, dtype=np.float32))


def dump_outputs(out_dir: str, loss, grads, params) -> None:
    """Write the last timed step's results as float32 .npy files."""
    os.makedirs(out_dir, exist_ok=True)
    _dump_array(os.path.join(out_dir, "loss.npy"), loss)
    _dump_array(os.path.join(out_dir, "grads.npy"), grads)
    _dump_array(os.path.join(out_dir, "params.npy"), params)


def main() -> None:
    _enable_tuned_gemms()
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's loss, gradients and "
                        "updated parameters to DIR/<name>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run measurements beyond the headline figure "
                        "(this benchmark has none)")
    args = p.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))

    from genrec_amd.models.tiger import Tiger
    from genrec_amd.parallel import init_distributed
    from genrec_amd.parallel.ddp import broadcast_parameters

    ctx = init_distributed()
    device = ctx.device
    use_gpu = device.type == "cuda"
    torch.manual_seed(1234)

    # reference TIGER Amazon-Beauty architecture (tiger.gin:16-25)
    cfg = dict(embedding_dim=128, attn_dim=384, dropout=0.1, num_heads=6,
               n_layers=8, num_item_embeddings=256, num_user_embeddings=10000,
               sem_id_dim=3)
    model = Tiger(**cfg).to(device)
    broadcast_parameters(model)

    n_items_hist = 20
    batches = [
        build_batch(args.batch_size, n_items_hist, cfg["sem_id_dim"],
                    cfg["num_item_embeddings"], cfg["num_user_embeddings"],
                    device, seed=100 + rank * 1000 + i)
        for i in range(8)
    ]

    # hipGraph capture of the whole train step (fwd+bwd+allreduce+clip+AdamW)
    # removes per-launch host overhead — the step is ~1000 tiny dispatches.
    # On capture failure (e.g. an RCCL build without graph support) the SAME
    # bf16/master-weight step runs eagerly, so N=1 and N>1 numbers stay
    # mode-comparable.
    use_graph = use_gpu and os.environ.get("GENREC_BENCH_GRAPH", "1") == "1"

    if use_gpu:
        # GraphedTrainStep: pure-bf16 model + ONE flat fp32 master/moment
        # buffer stepped by the genrec fused_adamw HIP kernel, bf16 flat
        # gradient all-reduced in a single RCCL message, whole step
        # hipGraph-captured (eager fallback on capture failure keeps N=1
        # and N>1 numbers mode-comparable).
        from genrec_amd.parallel.graph_runner import GraphedTrainStep

        runner = GraphedTrainStep(
            model, batches[0], lambda out: out.loss, lr=1e-4,
            weight_decay=0.035, clip_norm=1.0, world=world,
            use_graph=use_graph)
        use_graph = runner.captured
        nocopy = os.environ.get("GENREC_BENCH_NOCOPY", "0") == "1"

        def step(i: int):
            if nocopy and runner.captured:
                runner._graph.replay()
                return runner._loss
            return runner.step(batches[i % len(batches)])
    else:  # CPU path (driver's no-GPU contract check)
        from genrec_amd.parallel import GradReducer

        opt = torch.optim.AdamW(model.parameters(), lr=1e-4,
                                weight_decay=0.035)
        reducer = GradReducer(model)

        def step(i: int):
            b = batches[i % len(batches)]
            opt.zero_grad(set_to_none=False)
            out = model(**b)
            out.loss.backward()
            reducer.finalize()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            return out.loss

    model.train()
    for i in range(args.warmup):
        step(i)
    if use_gpu:
        # Training is chaotic: the step is not bitwise repeatable (a rare
        # one-ulp difference between runs, as float atomics give), and
        # hundreds of AdamW steps amplify that far beyond rounding
        # (measured: loss 13% apart after 1000 steps, one parameter 1 ulp
        # apart after 25). So that the LAST timed step computes
        # the same thing in every run, the model/optimizer/RNG state of
        # this point (it depends only on the arguments) is kept here and
        # put back, with the clock stopped, just before that step.
        from genrec_amd.ops.attention import _seed_counter

        torch.cuda.synchronize()
        state0 = (runner._opt_snapshot(), _seed_counter(device).clone(),
                  torch.cuda.get_rng_state(device), torch.get_rng_state())
    # Extra UNTIMED warmup until GPU clocks settle: a fresh box ramps
    # sclk over the first ~2 s of load; short driver settings (warmup 5)
    # otherwise time the ramp. The timed region below is still exactly
    # args.steps steps. The extra count is derived from ONE timed step
    # and MAX-agreed across ranks — every rank must run the same number
    # of steps (each contains a collective for N>1) or the job deadlocks.
    if use_gpu:
        torch.cuda.synchronize()
        t_w = time.perf_counter()
        step(args.warmup)
        torch.cuda.synchronize()
        dt = max(time.perf_counter() - t_w, 1e-4)
        n_extra = min(int(2.5 / dt), 2000)
        if world > 1:
            import torch.distributed as dist

            t = torch.tensor([n_extra], dtype=torch.int64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            n_extra = int(t.item())
        for i in range(n_extra):
            step(args.warmup + 1 + i)
        torch.cuda.synchronize()

    ctx.barrier()
    if use_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps - 1):
        step(args.warmup + i)
    elapsed = 0.0
    if use_gpu:
        # stop the clock, restore the kept state, restart the clock: the
        # last step is timed like the others and args.steps steps are
        # timed in all
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        runner._opt_restore(state0[0])
        _seed_counter(device).copy_(state0[1])
        torch.cuda.set_rng_state(state0[2], device)
        torch.set_rng_state(state0[3])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
    loss = step(args.warmup + args.steps - 1)
    if use_gpu:
        torch.cuda.synchronize()
    ctx.barrier()
    elapsed += time.perf_counter() - t0

    if args.dump_outputs and rank == 0:
        with torch.no_grad():
            if use_gpu:
                params = runner.flat_master if runner.fused else \
                    torch.cat([m.reshape(-1) for m in runner.masters])
                grads = runner.flat_grads
            else:
                ps = list(model.parameters())
                params = torch.cat([q.reshape(-1) for q in ps])
                grads = torch.cat([
                    (q.grad if q.grad is not None else torch.zeros_like(q))
                    .reshape(-1) for q in ps])
            dump_outputs(args.dump_outputs, loss, grads, params)

    # MAX over ranks
    if world > 1:
        import torch.distributed as dist

        t = torch.tensor([elapsed], dtype=torch.float64, device=device
                         if use_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    global_batch = args.batch_size * world
    samples_per_s = global_batch * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank == 0:
        print(json.dumps({
            "metric": "train_samples_per_s",
            "value": samples_per_s,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_gpu else "fp32",
            "data": "synthetic",
            "config": {
                "model": "tiger-amazon-beauty",
                "global_batch": global_batch,
                "seq_len": n_items_hist * cfg["sem_id_dim"] + 1,
                "parallelism": f"dp{world}",
                "hip_graph": bool(use_graph),
            },
        }))


if __name__ == "__main__":
    main()
