"""Time the bilinear 2x launches of the DPT heads on the headline's shapes (42 pairs, 512x384) in both kernel forms, same process,
alternating, and print a digest of every output (the forms are bitwise equal: tests/test_gpu_up2x_forms.py)."""
import ctypes as C, hashlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from align3r_amd import _lib, ops
lib = _lib.load()
p = lambda t: C.c_void_p(t.data_ptr())
def timeit(fn, iters=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3
def sha(*ts):
    h = hashlib.sha1()
    for t in ts: h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:12]
g = torch.Generator(device="cuda").manual_seed(1)
rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
def fh2_case(B, H, W, Cc):
    x, y, word = rnd(B, H, W, Cc), torch.zeros(B * 4 * H * W * Cc * 4, dtype=torch.uint8, device="cuda"), ops.absmax_word("cuda")
    f = lambda: lib.a3r_upsample2x_fh2(p(x), p(y), B, H, W, Cc, 2 * H, 2 * W, 1.0, p(word), _lib.stream_ptr())
    return f"fh2 [{B},{H},{W},{Cc}]", f, lambda: sha(y, word), 4.0 * B * H * W * Cc * 5
def f32_case(B, H, W, Cc):
    x, y = rnd(B, H, W, Cc), torch.zeros(B, 2 * H, 2 * W, Cc, device="cuda")
    f = lambda: lib.a3r_upsample2x(p(x), p(y), B, H, W, Cc, 2 * H, 2 * W, _lib.stream_ptr())
    return f"f32 [{B},{H},{W},{Cc}]", f, lambda: sha(y), 4.0 * B * H * W * Cc * 5
def combine_case(S, U, H, W, Cc):
    x, c, r0 = rnd(S, H, W, Cc), rnd(U, 2 * H, 2 * W, Cc), rnd(U, 2 * H, 2 * W, Cc)
    m = (torch.arange(S, device="cuda") % U).int()
    s, sr2, word = torch.zeros(S, 2 * H, 2 * W, Cc, device="cuda"), torch.zeros(S * 4 * H * W * Cc * 4, dtype=torch.uint8, device="cuda"), ops.absmax_word("cuda")
    f = lambda: lib.a3r_upsample2x_combine_fh2(p(x), p(c), p(r0), p(m), p(s), p(sr2), S, H, W, Cc, 2 * H, 2 * W, 1.0, p(word), _lib.stream_ptr())
    return f"combine [{S}<-{U},{H},{W},{Cc}]", f, lambda: sha(s, sr2, word), 4.0 * H * W * Cc * (S * 9 + U * 8)
for make in (lambda: fh2_case(42, 192, 256, 128), lambda: fh2_case(42, 96, 128, 256), lambda: combine_case(42, 15, 48, 64, 256),
             lambda: f32_case(42, 24, 32, 256)):
    name, f, dig, nbytes = make()
    for rep in range(2):
        for form in (1, 2):
            lib.a3r_upsample2x_set_form(form)
            assert f() == 0
            torch.cuda.synchronize()
            d = dig()
            us = timeit(f)
            print(f"{name:>28s} form {form}: {us:8.1f} us {nbytes / us / 1e6:5.2f} TB/s  sha {d}", flush=True)
    lib.a3r_upsample2x_set_form(2)
    del f, dig
    torch.cuda.empty_cache()
