"""Generate tests/golden/vae_encode.npz from the reference's own modules (runs only where the reference is present).

    DUODIFF_REFERENCE=/path/to/reference python tools/gen_vae_encode_golden.py

FrozenAutoencoderKL.encode_moments / sample (models/utils/autoencoder.py:468-479) with the reference's Encoder, a
torch.nn.Conv2d(8, 8, 1) as quant_conv and the seeded synthetic weights of synthetic_vae_encoder_state_dict.  The file holds
data only (inputs, outputs, seeds, counts), no weights:

  seed                 the encoder weights' seed
  n_tensors, n_values  the encode side's tensor / value count, as the reference's modules report them
  x64, moments8        [2,3,64,64] uniform in [-1, 1] and its moments [2,8,8,8]
  x256_seed, moments32 the generator seed of a [1,3,256,256] uniform input and its whole moments [1,8,32,32]
  stats8, stats32      mean, std, min, max of the two outputs
  sample_moments       [2,8,4,4] hand-made moments: logvar entries below -30, above 20 and in between
  sample_seed          the torch.manual_seed value in front of the reference's sample()
  sample_z, sample_eps the reference's z and the randn_like(mean) draw that seed gives
"""
import contextlib
import io
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
REF = Path(os.environ.get("DUODIFF_REFERENCE", ""))
OUT = REPO / "tests" / "golden"
SEED, X64_SEED, X256_SEED, SAMPLE_SEED = 8765, 71, 72, 1234

sys.dont_write_bytecode = True


def uniform_image(shape, seed):
    """uniform in [-1, 1], as images are (tests/test_vae_encode.py draws the 256 x 256 input the same way)"""
    return 2.0 * torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 1.0


def main():
    if not os.environ.get("DUODIFF_REFERENCE") or not (REF / "models" / "utils" / "autoencoder.py").exists():
        raise SystemExit("reference not found: set DUODIFF_REFERENCE to its checkout")
    sys.path.insert(0, str(REPO))
    sys.path.insert(0, str(REF))
    from duodiff_amd.autoencoder import synthetic_vae_encoder_state_dict
    from models.utils.autoencoder import Encoder, FrozenAutoencoderKL
    ddconfig = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                    num_res_blocks=2, attn_resolutions=[], dropout=0.0)
    with contextlib.redirect_stdout(io.StringIO()):
        enc = Encoder(**ddconfig).eval()
    qc = torch.nn.Conv2d(8, 8, 1).eval()
    sd = synthetic_vae_encoder_state_dict(SEED)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
    qc.load_state_dict({"weight": sd["quant_conv.weight"], "bias": sd["quant_conv.bias"]})
    mods = list(enc.state_dict().values()) + list(qc.state_dict().values())
    out = dict(seed=np.array(SEED), n_tensors=np.array(len(mods)), n_values=np.array(sum(t.numel() for t in mods)))

    def stats(a):
        return np.array([a.mean(dtype=np.float64), a.std(dtype=np.float64), a.min(), a.max()])

    torch.set_num_threads(8)
    with torch.no_grad():
        x64 = uniform_image((2, 3, 64, 64), X64_SEED)
        m8 = qc(enc(x64)).numpy()
        m32 = qc(enc(uniform_image((1, 3, 256, 256), X256_SEED))).numpy()
        out.update(x64=x64.numpy(), moments8=m8, stats8=stats(m8), x256_seed=np.array(X256_SEED), moments32=m32, stats32=stats(m32))
        # sample(): hand-made moments whose logvar crosses both clamps
        g = torch.Generator().manual_seed(SAMPLE_SEED + 1)
        mo = torch.randn(2, 8, 4, 4, generator=g)
        lv = torch.tensor([-100.0, -30.0, -29.5, -3.0, 0.0, 2.5, 19.5, 20.0, 25.0, 80.0, -31.0, 1.0, -0.5, 5.0, -12.0, 21.0])
        mo[0, 4:] = lv.reshape(1, 4, 4) + torch.arange(4).reshape(4, 1, 1) * 0.25
        mo[1, 4:] = 6.0 * mo[1, 4:]
        torch.manual_seed(SAMPLE_SEED)
        z = FrozenAutoencoderKL.sample(types.SimpleNamespace(scale_factor=0.18215), mo)
        torch.manual_seed(SAMPLE_SEED)
        eps = torch.randn_like(mo[:, :4])
        out.update(sample_moments=mo.numpy(), sample_seed=np.array(SAMPLE_SEED), sample_z=z.numpy(), sample_eps=eps.numpy())
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez(OUT / "vae_encode.npz", **out)
    size = (OUT / "vae_encode.npz").stat().st_size
    print(f"vae_encode.npz: {size} bytes; tensors {int(out['n_tensors'])}, values {int(out['n_values'])}; moments8 std {m8.std():.4f}, "
          f"moments32 std {m32.std():.4f}")
    assert size <= (OUT / "vae_decode.npz").stat().st_size, "larger than vae_decode.npz"


if __name__ == "__main__":
    main()
