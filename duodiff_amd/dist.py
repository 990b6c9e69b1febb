"""Multi-GPU sampling: one process per GPU, batches sharded with no collective inside the loop.

Images are independent (no cross-sample reduction anywhere on the path: LayerNorm and softmax are
per token / per row), so the 1000-step loop shards embarrassingly: rank r samples its own batch
with ``seed = base_seed + r``, which is bit-for-bit what the r-th independent reference invocation
``sampler.py --seed base_seed+r --batch_size B`` computes (the reference has no notion of a global
batch).  Exactly ONE collective closes a run: the gather of the finished images
(RCCL over xGMI when the backend is "nccl", gloo on CPU for tests).

With ``--image_seeds`` the run is instead ONE set of pictures, image i under seed ``base_seed + first_image + i``: every rank keeps
the base seed and rank r samples images ``first_image + r B ...``, so the gathered W x B images equal one rank's run of W B images, and
any image can be regenerated alone (``--first_image i --batch_size 1``).

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m duodiff_amd.dist --config_path ... (same flags as sampler)
"""
import os
from typing import Callable, Optional

import numpy as np
import torch
import torch.distributed as dist


def env_rank():
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


def init(backend: Optional[str] = None):
    """Initialise torch.distributed from the torchrun environment (no-op for a single process)."""
    rank, world, local = env_rank()
    if world == 1:
        return rank, world, local
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend is None:
        # DUODIFF_DIST_BACKEND=gloo forces the CPU transport (rehearsing N ranks on one GPU; tests)
        backend = os.environ.get("DUODIFF_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return rank, world, local


def rank_seed(base_seed: int, rank: int) -> int:
    """Seed of rank r's shard: the r-th independent single-GPU run."""
    return int(base_seed) + int(rank)


def rank_first_image(first_image: int, rank: int, batch_size: int) -> int:
    """--image_seeds: the first image of rank r's shard within the whole run"""
    return int(first_image) + int(rank) * int(batch_size)


def gather_images(local: torch.Tensor, world: int, dst: Optional[int] = None):
    """The single collective: all ranks' [B,H,W,C] images, in rank order.

    dst=None -> all_gather (every rank gets [world*B,H,W,C]); dst=k -> gather to rank k only
    (others get None).  With the nccl backend this is ncclAllGather / ncclGather over xGMI:
    6.3 MB per rank for CelebA B=128, once per >= 1000 steps.
    """
    if world == 1:
        return local
    local = local.contiguous()
    if dist.get_backend() == "gloo" and local.is_cuda:
        local = local.cpu()          # gloo moves host memory; the payload is one image batch per >= 1000 steps
    if dst is None:
        out = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(out, local)
        return torch.cat(out, dim=0)
    rank = dist.get_rank()
    out = [torch.empty_like(local) for _ in range(world)] if rank == dst else None
    dist.gather(local, gather_list=out, dst=dst)
    return torch.cat(out, dim=0) if rank == dst else None


def sample_sharded(sample_fn: Callable[[int], torch.Tensor], base_seed: int, dst: Optional[int] = None,
                   barrier: bool = True, rank_seeds: bool = True):
    """Run ``sample_fn(seed)`` (one rank's whole sampling loop, returning [B,H,W,C] images) on every
    rank with its own seed, then gather.  No communication happens inside ``sample_fn``.
    rank_seeds=False (per-image seeds): every rank gets the base seed; ``sample_fn`` names its shard by its first image.

    Returns (gathered images or None on non-destination ranks, this rank's local images).
    """
    rank, world, _ = env_rank()
    if world > 1 and not dist.is_initialized():
        raise RuntimeError("call duodiff_amd.dist.init() first")
    local = sample_fn(rank_seed(base_seed, rank) if rank_seeds else int(base_seed))
    if not torch.is_tensor(local):
        local = torch.from_numpy(np.asarray(local))
    if world > 1 and barrier:
        dist.barrier()
    return gather_images(local, world, dst), local


def main(argv=None):
    """Sharded version of the sampler CLI: its flags and its run setup (sampler.setup_run); --batch_size is per GPU; rank 0 writes the
    output.  Not taken: the image-to-image and inpainting flags, and --timesteps_save (intermediates are not gathered)."""
    import time
    from pathlib import Path

    from . import sampler
    args = sampler.get_args(argv)
    if any(v is not None for v in (args.init_image, args.strength, args.known_image, args.known_mask)) or args.encode_images:
        raise ValueError("--init_image / --strength / --known_image / --known_mask / --encode_images belong to the single-GPU sampler (duodiff_amd.sampler)")
    if args.timesteps_save:
        raise ValueError("--timesteps_save belongs to the single-GPU sampler (duodiff_amd.sampler): intermediates are not gathered")
    rank, world, local_rank = init()
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank % torch.cuda.device_count())   # (ranks may share a GPU when rehearsed on one)
    setup = sampler.setup_run(args)

    def one_rank(seed):
        # --image_seeds: `seed` is the base seed on every rank (below) and the shard is named by its first image
        image_seeds = sampler.image_seed_list(args, args.batch_size, rank_first_image(args.first_image, rank, args.batch_size))
        sampler.seed_everything(seed)               # (get_samples seeds again: a run without labels is what it was)
        y = sampler.labels_from_args(args, args.batch_size, setup.mp.num_classes, image_seeds)   # same draw and range check as the single-GPU CLI
        return sampler.get_samples(**setup.kwargs, seed=seed, image_seeds=image_seeds, y=y, timesteps_save=[], return_device_tensor=True)[0]

    tic = time.time()
    allimgs, _ = sample_sharded(one_rank, args.seed, dst=0, rank_seeds=not args.image_seeds)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    tac = time.time()
    if rank == 0:
        out = Path(args.output_folder)
        out.mkdir(parents=True, exist_ok=True)
        imgs = allimgs.cpu().numpy()
        sampler.dump_statistics(tac - tic, out, imgs.shape[0])
        if args.no_png:
            np.save(out / "samples.npy", imgs)
        else:
            sampler.dump_samples(imgs, out)
        print(f"Elapsed time: {tac - tic} s  ({imgs.shape[0] / (tac - tic):.3f} images/s on {world} GPU(s))")
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
