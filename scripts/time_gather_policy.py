"""Load policy of the batch gather (csrc/dataset.hip): non-temporal loads (the product library) against default-policy loads (the
ablation build, switch 16384), the same entry point called the same way (ctypes) for both, over B = 16 ... 256 at 144 x 160 on a
bank of 4096 rows.  Per B, medians in microseconds of: one launch between HIP events on an idle stream (`nt`, `plain`; 100 after
20, the order of the two alternating per iteration), and per-launch time of 20 launches back to back (`*_train`; 20 trains after
4): python scripts/time_gather_policy.py [--out profiles/dataset_gather_policy.json]"""
import ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import unet_rir_amd as U
DEV = torch.device("cuda:0")
H, W, N = 144, 160, 4096
L = U._lib.lib()
_src = [os.path.join(U.build.CSRC, f) for f in os.listdir(U.build.CSRC)]
if not os.path.exists(U.build.ABL_LIB) or any(os.path.getmtime(s) > os.path.getmtime(U.build.ABL_LIB) for s in _src):
    U.build.build_ablations()
A = C.CDLL(U.build.ABL_LIB); A.unetrir_abl_set(16384)
fa = U._lib.bind(A, "unetrir_gather_batch_f32")
fn_ = L.unetrir_gather_batch_f32
g = torch.Generator(device=DEV).manual_seed(1)
bank = torch.rand((N, 2, H, W), device=DEV, generator=g)
emb_bank = torch.randint(26, 1282, (N, 16), device=DEV, generator=g, dtype=torch.int32)
p = lambda t: C.c_void_p(t.data_ptr())
out = {}
for B in (16, 32, 64, 128, 256):
    idx = torch.randint(0, N, (24, 2, B), device=DEV, generator=g, dtype=torch.int32)
    a, b = (torch.empty((B, 2, H, W), device=DEV) for _ in range(2))
    e = torch.empty((B, 2, 16), dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    def call(f, k):
        assert f(p(bank), N, 2 * H * W, p(emb_bank), 16, None, 0, None, p(idx[k, 0]), p(idx[k, 1]), B, p(a), p(b), p(e), None, None, st) == 0
    res = {"nt": [], "plain": [], "nt_train": [], "plain_train": []}
    for it in range(120):
        order = (("nt", fn_), ("plain", fa)) if it % 2 == 0 else (("plain", fa), ("nt", fn_))
        evs = []
        for name, f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(f, it % 24); e1.record(); evs.append((name, e0, e1))
        torch.cuda.synchronize()
        if it >= 20:
            for name, e0, e1 in evs: res[name].append(e0.elapsed_time(e1))
    for it in range(24):          # trains: 20 launches back to back, per-launch time (launch gaps hidden behind the queue)
        order = (("nt", fn_), ("plain", fa)) if it % 2 == 0 else (("plain", fa), ("nt", fn_))
        for name, f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(20): call(f, (it + k) % 24)
            e1.record(); torch.cuda.synchronize()
            if it >= 4: res[name + "_train"].append(e0.elapsed_time(e1) / 20)
    out[B] = {k: round(statistics.median(v) * 1e3, 2) for k, v in res.items()}
    print(B, out[B], "us", flush=True)
dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "profiles/dataset_gather_policy.json"
os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
json.dump(out, open(dst, "w"), indent=1)
