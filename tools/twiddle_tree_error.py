"""Error of the twiddle powers of a float radix-32 stage (fft_tiled.h TWMODE 3, the stage fft_fir32.h runs twice per block): one correctly
rounded base twiddle w per butterfly and w^2 .. w^31 recomputed by the kernel's product tree, against correctly rounded table entries.
The rounding error of w grows with the exponent (w^q about q/5.6 eps RMS); DESIGN.md §4.1 quotes the figures.  CPU only:

    python tools/twiddle_tree_error.py
"""
import numpy as np
f = np.complex64
def cm(a, b): return (a * b).astype(f)
n = 8192; R = 32
ks = np.arange(n // R)                       # base angles of the butterflies: w = W_n^k
w = np.exp(-2j * np.pi * ks / n).astype(f)
p = [None] * 32
p[1] = w; p[2] = cm(p[1], p[1]); p[3] = cm(p[2], p[1])
p[4] = cm(p[2], p[2]); p[5] = cm(p[4], p[1]); p[6] = cm(p[3], p[3]); p[7] = cm(p[4], p[3])
p[8] = cm(p[4], p[4]); p[9] = cm(p[8], p[1]); p[10] = cm(p[5], p[5]); p[11] = cm(p[8], p[3])
p[12] = cm(p[6], p[6]); p[13] = cm(p[8], p[5]); p[14] = cm(p[7], p[7]); p[15] = cm(p[8], p[7])
p16 = cm(p[8], p[8]); p[16] = p16
for q in range(1, 16): p[16 + q] = cm(p16, p[q])
eps = np.finfo(np.float32).eps
tree, table = [], []
for q in range(1, 32):
    ex = np.exp(-2j * np.pi * q * ks / n)
    tree.append(np.abs(p[q].astype(complex) - ex)); table.append(np.abs(ex.astype(f).astype(complex) - ex))
tree, table = np.concatenate(tree), np.concatenate(table)
print(f"radix-32 powers: product tree RMS {np.sqrt((tree**2).mean())/eps:.2f} eps, max {tree.max()/eps:.2f} eps; "
      f"table RMS {np.sqrt((table**2).mean())/eps:.2f} eps, max {table.max()/eps:.2f} eps")
for q in (1, 2, 4, 8, 15, 16, 31):
    ex = np.exp(-2j * np.pi * q * ks / n)
    d = np.abs(p[q].astype(complex) - ex)
    print(f"  w^{q:2d}: RMS {np.sqrt((d**2).mean())/eps:.2f} eps")
