"""Recurrence launch time against the number of sequences (one chain per CU up to 128 rows): python tools/time_gru_rows.py"""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import torch
from mm_dfn_amd import gru as fused, _hip
H = 100
dev = "cuda"
def run(T, rows, iters=30):
    gi = torch.randn(T, rows, 600, device=dev)
    whh = [torch.randn(300, 100, device=dev) * 0.1 for _ in range(2)]
    bhh = [torch.randn(300, device=dev) * 0.1 for _ in range(2)]
    y = torch.empty(T, rows, 200, device=dev); g = torch.empty(T, rows, 2, 4, 100, device=dev)
    dy = torch.randn(T, rows, 200, device=dev); dgi = torch.empty(T, rows, 600, device=dev); dgh = torch.empty_like(dgi)
    lib = _hip.lib()
    def f():
        lib.mmdfn_gru_seq_fwd(1, _hip.ptr_array([gi]), _hip.ptr_array(whh), _hip.ptr_array(bhh), _hip.ptr_array([y]), _hip.ptr_array([g]), _hip.int_array([rows]), _hip.int_array([T]), H, None, _hip.stream())
    def b():
        lib.mmdfn_gru_seq_bwd(1, _hip.ptr_array([dy]), _hip.ptr_array([y]), _hip.ptr_array([g]), _hip.ptr_array(whh), _hip.ptr_array([dgi]), _hip.ptr_array([dgh]), _hip.int_array([rows]), _hip.int_array([T]), H, None, _hip.stream())
    out = []
    for fn in (f, b):
        for _ in range(10): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters * 1e3)
    return out
for T in (110, 33):
    for rows in (1, 16, 40, 80, 100, 120, 128, 160, 256):
        f, b = run(T, rows)
        print("T=%d rows=%d chains=%d fwd %.1f us (%.3f/step) bwd %.1f us (%.3f/step)" % (T, rows, 2 * rows, f, f / T, b, b / T))
