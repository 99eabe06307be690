"""What the tools/*_host.py tools share: the stand-in for <hip/hip_runtime.h> the headers of csrc/ are compiled against on the host (the
hardware's rcp / rsq / exp / log become the C library's, erfcx is exp(x^2) erfc(x) in float64), the host compiler call that makes a tool's
MAIN a stand-alone program (optionally under AddressSanitizer and UndefinedBehaviorSanitizer), the binary exchange of the two HMC programs,
and the tools' command line.  Each tool keeps its own MAIN, its evaluate / run / solve and its survey."""
import argparse
import json
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesflow_nddms_amd", "csrc")

SHIM = r"""#pragma once
#include <cmath>
#include <cstring>
#include <cstdint>
#include <math.h>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct float2 { float x, y; };
inline float2 make_float2(float a, float b) { return {a, b}; }
struct dim3s { unsigned x, y, z; };
static dim3s threadIdx, blockIdx;
inline void __syncthreads() {}
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_rsqf(x) (1.0f / sqrtf(x))
#define __builtin_amdgcn_exp2f(x) exp2f(x)
#define __builtin_amdgcn_logf(x) log2f(x)
#define __builtin_amdgcn_readlane(x, k) (x)
inline float __expf(float x) { return expf(x); }
inline float __logf(float x) { return logf(x); }
inline float erfcxf(float xf) {
    double x = xf;
    if (x < 25.0) return (float)(exp(x * x) * erfc(x));
    double i2 = 1.0 / (x * x);
    return (float)(0.5641895835477563 / x * (1.0 - 0.5 * i2 + 0.75 * i2 * i2));
}
inline float sinpif(float x) { return (float)sin(M_PI * (double)x); }
inline float cospif(float x) { return (float)cos(M_PI * (double)x); }
inline unsigned __float_as_uint(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
template <class T> inline T __shfl_xor(T s, int, int) { return s; }
"""


def build(td, main, name, sanitize=False):
    """Compile the program `main` against the stand-in header into td -> the path of the program `name`."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler found")
    os.makedirs(os.path.join(td, "hip"))
    with open(os.path.join(td, "hip", "hip_runtime.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(td, "main.cpp"), "w") as f:
        f.write(main)
    exe = os.path.join(td, name)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call([cxx, "-std=c++17", "-w"] + flags + ["-I", td, "-I", CSRC, "-o", exe, os.path.join(td, "main.cpp")])
    return exe


def exchange(exe, header, arrays, table):
    """The HMC programs' exchange: `header` as int64 words and then `arrays` go to in.bin beside the program, the program runs, and out.bin
    is cut by `table` = ((key, dtype, shape), ...) in the file's order, which must account for its whole length -> {key: array}."""
    fin, fout = os.path.join(os.path.dirname(exe), "in.bin"), os.path.join(os.path.dirname(exe), "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array(header, np.int64).tobytes())
        for a in arrays:
            f.write(a.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    o, out = 0, {}
    for key, dt, shape in table:
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[key] = np.frombuffer(raw[o:o + n], dt).reshape(shape).copy()
        o += n
    assert o == len(raw)
    return out


def cli(survey, rows=None):
    """A tool's command line: [--sanitize] [--json OUT], and [--rows N] where the survey takes a number of rows (`rows`: its default);
    prints survey's result as one JSON line and writes it to OUT."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    if rows is not None:
        ap.add_argument("--rows", type=int, default=rows)
    ap.add_argument("--json")
    a = ap.parse_args()
    line = json.dumps(survey(a.sanitize) if rows is None else survey(a.sanitize, a.rows))
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
