#!/bin/bash
# Rebuild libsola with gemm_glds.hip's DEVICE code taken from an (edited) assembly file - the ISA bisection of the fused GroupNorm epilogue's fault.
# (gemm_glds.o holds the one-tile and the persistent NT kernels, the fused epilogue among them; gemm_tn_tr_kernel is in gemm_tn_tr.o, the k16 and
# ping-pong experiments in build/obj_exp/lab_gemm_*.o)
#   tools/asm_rebuild.sh <device.s> <host object with the same kernels> <out.so>
set -e
L=/opt/rocm/lib/llvm/bin
S=$1; HOSTOBJ=$2; OUT=$3
T=$(mktemp -d)
$L/clang -x assembler -target amdgcn-amd-amdhsa -mcpu=gfx950 -c "$S" -o $T/dev.o
$L/ld.lld -shared $T/dev.o -o $T/dev.co
$L/clang-offload-bundler --type=o --targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950 --input=/dev/null --input=$T/dev.co --output=$T/fat.bin
$L/llvm-objcopy --update-section .hip_fatbin=$T/fat.bin "$HOSTOBJ" $T/gemm_glds.o
OBJS=$(ls /root/repo/build/obj/*.o | grep -v gemm_glds.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" $OBJS $T/gemm_glds.o
rm -rf $T
