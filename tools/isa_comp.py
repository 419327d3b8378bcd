#!/usr/bin/env python3
"""tools/isa_comp.py [-DFLAG ...] — gfx950 instruction counts of the two-stage compositor's stage B and of Overwrite, compiled alone.

One probe kernel per composite (k_blend.h: comp_nx<OB> on one pixel per lane, the blend function's three results read from memory
like the pixel) and one for blend_nx<Overwrite, 0>, with the library's flags for k_flatten.hip; a probe that composites nothing gives the
harness's own instructions, which are subtracted.  Prints VALU instructions and how many of them are v_cndmask / v_cmp.  Extra arguments
go to the compiler (-DPFX_WB_MASK=0 and the like).  No GPU needed (cross-compile only)."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math",
         "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize", "--offload-arch=gfx950", "--cuda-device-only", "-S"]

SRC = r'''
#include "k_blend.h"
using namespace pfxk;
// K: 0 .. 2 = comp_nx<K>, 3 = blend_nx<Overwrite, 0>, -1 = the harness alone
template <int K>
__global__ __launch_bounds__(256) void probe(const float4* __restrict__ top, const float4* __restrict__ fs, float* __restrict__ accs, float opc, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const float4 v = top[i], g = fs[i];
    // the accumulator channels come and go as four separate dwords (planar): a float4 would tie them to a register quad, and the moves between the load's
    // quad and the store's would be counted as the composite's (in the kernels the accumulators live in registers across the layer loop)
    float acc[4] = {accs[i], accs[n + i], accs[2u * n + i], accs[3u * n + i]};
    const float t[4] = {v.x, v.y, v.z, v.w}, f[3] = {g.x, g.y, g.z};
    if constexpr (K == 3) blend_nx<M_OVERWRITE, 0>(acc, t, opc, opc);
    else if constexpr (K >= 0) comp_nx<K>(acc, t, f, opc);
    else acc[0] += t[0] + t[1] + t[2] + t[3] + f[0] + f[1] + f[2] + opc;
    accs[i] = acc[0]; accs[n + i] = acc[1]; accs[2u * n + i] = acc[2]; accs[3u * n + i] = acc[3];
}
template __global__ void probe<-1>(const float4*, const float4*, float*, float, uint32_t);
template __global__ void probe<0>(const float4*, const float4*, float*, float, uint32_t);
template __global__ void probe<1>(const float4*, const float4*, float*, float, uint32_t);
template __global__ void probe<2>(const float4*, const float4*, float*, float, uint32_t);
template __global__ void probe<3>(const float4*, const float4*, float*, float, uint32_t);
'''
NAMES = {0: "comp_nx<0> general", 1: "comp_nx<1> opaque accumulator", 2: "comp_nx<2>", 3: "blend_nx<Overwrite, 0>"}


def main():
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "probe.hip")
        open(f, "w").write(SRC)
        asm = os.path.join(td, "probe.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *sys.argv[1:], "-I", os.path.join(ROOT, "paintfe_amd", "csrc"), "-I",
                               os.path.join(ROOT, "include"), "-o", asm, f], stderr=subprocess.DEVNULL)
        text = open(asm).read()
    counts = {}
    for mm in re.finditer(r"^_Z5probeILi(n?\d+)EEvPK15HIP_vector_typeIfLj4EES3_Pffj:(.*?)s_endpgm", text, re.S | re.M):
        k, body = int(mm.group(1).replace("n", "-")), mm.group(2)
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.strip() and not l.strip().startswith((";", "."))]
        counts[k] = (sum(1 for i in ins if i.startswith("v_")), sum(1 for i in ins if i.startswith("v_cndmask")),
                           sum(1 for i in ins if i.startswith("v_cmp")), sum(1 for i in ins if i.startswith("v_mov")), sum(1 for i in ins if i.startswith("s_") and not i.startswith(("s_waitcnt", "s_nop", "s_load", "s_endpgm"))))
    base_v = counts[-1][0] - 8   # the empty probe's own eight adds
    base_s = counts[-1][4]
    base_m = counts[-1][3]
    print("| composite | VALU | of which v_cndmask | v_cmp | v_mov | SALU |\n|---|---|---|---|---|---|")
    for key, name in NAMES.items():
        v, c, p, m, s = counts[key]
        print(f"| {name} | {v - base_v} | {c} | {p} | {m - base_m} | {s - base_s} |")


if __name__ == "__main__":
    main()
