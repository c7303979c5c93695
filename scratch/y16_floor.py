# K1's skeleton (proxmin_amd/csrc/bench_floor.hip) with the 8-byte and the 16-byte Y fetches, burst and spread over the slot, with and without the
# producers' epilogue: the prediction for k_grad_f16_v8<.., Y16>.  Same arguments as bench.py's peaks leg (16384 x 16384, random data, 20 launches
# x 2 passes per call); the variants alternate and every one runs REPS times.        usage: python scratch/y16_floor.py [REPS] > profiles/y16_floor.txt
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = C.CDLL(os.path.join(ROOT, "proxmin_amd", "libpmx_floor.so"))
lib.pmxf_stream.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
lib.pmxf_last_error.restype = C.c_char_p
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
VARIANTS = [(1111, "epilogue  8 B/lane, a pair's 16 requests in one burst"), (1112, "epilogue  16 B/lane, one block per 4 requests (burst)"),
            (1114, "epilogue  16 B/lane spanning the pair + exchange, spread"), (1115, "epilogue  8 B/lane, spread (4 per MFMA)"),
            (1011, "no epi    8 B/lane, burst"), (1012, "no epi    16 B/lane, burst"),
            (1014, "no epi    16 B/lane spanning the pair + exchange, spread"), (1015, "no epi    8 B/lane, spread")]
ms = {v: [] for v, _ in VARIANTS}
for rep in range(REPS):
    for v, _ in VARIANTS:
        out = C.c_double()
        if lib.pmxf_stream(0, v, 16384, 16384, 0, 20, C.byref(out)) != 0:
            sys.exit("variant %d: %s" % (v, lib.pmxf_last_error().decode()))
        ms[v].append(out.value)
        print("# rep %d variant %d %.4f ms" % (rep, v, out.value), flush=True)
print("K1 skeleton, 16384 x 16384, 4 + 24 MFMAs per producer + consumer wave and block on random LDS operands; ms per launch, %d alternating repetitions" % REPS)
print("%-8s %-62s %s   min    median" % ("variant", "what", "  ".join("rep%d  " % i for i in range(REPS))))
for v, what in VARIANTS:
    x = sorted(ms[v])
    print("%-8d %-62s %s   %.4f %.4f" % (v, what, "  ".join("%.4f" % t for t in ms[v]), x[0], x[len(x) // 2]))
for a, b, what in ((1114, 1115, "16 B spanning vs 8 B, both spread, with epilogue"), (1014, 1015, "16 B spanning vs 8 B, both spread, no epilogue"),
                   (1112, 1111, "16 B vs 8 B, bursts, with epilogue (the comparison of the round-6 records)"), (1115, 1111, "8 B spread vs 8 B burst, with epilogue")):
    ma, mb = sorted(ms[a])[len(ms[a]) // 2], sorted(ms[b])[len(ms[b]) // 2]
    print("median %d / %d = %.4f   (%s)" % (a, b, ma / mb, what))
