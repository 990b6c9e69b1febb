"""Time dd_vae_encode beside dd_vae_decode on synthetic weights (ImageNet-256 latent geometry: 256x256x3 <-> 32x32x4), with device
events after a warm-up call: one image and a chunk of 4.

    python tools/vae_encode_bench.py [bf16|fp32] [iters]
"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from duodiff_amd.autoencoder import FrozenAutoencoderKL, synthetic_vae_encoder_state_dict, synthetic_vae_state_dict

prec = sys.argv[1] if len(sys.argv) > 1 else "bf16"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sd = synthetic_vae_state_dict()
sd.update(synthetic_vae_encoder_state_dict())
ae = FrozenAutoencoderKL(sd, precision=prec, max_chunk=4).to("cuda:0")


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


for B in (1, 4):
    x = (2 * torch.rand(B, 3, 256, 256) - 1).cuda()
    z = torch.randn(B, 4, 32, 32, device="cuda")
    te = timed(lambda: ae.encode_moments(x))
    td = timed(lambda: ae.decode(z))
    print(f"vae {prec} B={B}: encode_moments {te:.2f} ms ({te / B:.2f} ms/image)  decode {td:.2f} ms ({td / B:.2f} ms/image)", flush=True)
