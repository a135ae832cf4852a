"""Error of the stem's composite gradient (csrc/stem_composite.hip) and of the path it replaces (64 -> 64 data gradient, rounded to
bf16, then the stem's weight gradient and a column sum) against the fp64 formulas on the same bf16 inputs: relative L2 per tensor.
python scripts/stem_composite_error.py [B H W]        (default 2 256 256; prints one JSON line)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from unet_rir_amd import ops
import stem_composite_ref as SC

B, H, W = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (2, 256, 256)
dev = "cuda:0"
gen = torch.Generator().manual_seed(7)
x = torch.rand((B, H, W, 2), generator=gen).to(torch.bfloat16)
g = (torch.randn((B, H, W, 64), generator=gen) * 1e-3).to(torch.bfloat16)
w1 = (torch.randn((64, 3, 3, 64), generator=gen) / 24.0).to(torch.bfloat16)
xa = ops.Act(torch.zeros((B, H, W, 8), dtype=torch.bfloat16, device=dev)); xa.base[..., :2] = x.to(dev)
ga = ops.Act(g.to(dev).contiguous())
w1t = w1.permute(3, 1, 2, 0).contiguous().to(dev)
want_w, want_b = SC.stem_composite(x.double().numpy(), g.double().numpy(), w1.double().numpy())
rel = lambda a, r: float(np.linalg.norm(a.double().cpu().numpy() - r) / np.linalg.norm(r))
ws = ops.Workspace(dev)
dw, db = torch.zeros((64, 3, 3, 8), device=dev), torch.zeros(64, device=dev)
ops.stem_composite(ga, xa, w1t, dw, db, ws)
torch.cuda.synchronize()
new = {"dW0": rel(dw[..., :2], want_w), "db0": rel(db, want_b)}
gd = ops.new_act(B, H, W, 64, dev, dtype=torch.bfloat16)
ops.conv2d_dgrad(ops.geom(B, H, W, 64, 64, 3, 1), ga, w1t, gd)
ops.conv2d_wgrad(ops.geom(B, H, W, 8, 64, 3, 1), xa, gd, dw, ws)
ops.colsum(gd, db, ws)
torch.cuda.synchronize()
old = {"dW0": rel(dw[..., :2], want_w), "db0": rel(db, want_b)}
print(json.dumps({"shape": [B, H, W], "reference": "fp64 formulas (tests/stem_composite_ref.py) on the same bf16 inputs", "measure": "relative L2",
                  "composite": new, "replaced_path": old, "ratio": {k: new[k] / old[k] for k in new}}))
