#!/bin/bash
# Builds an A/B arm of the library that differs from the shipped one only in the cache policy of the forward chain's output stores
# (StorePolicy, mode_diffusion_policy_amd/csrc/mode_common.h):
#   scripts/build_store_variant.sh <tag> -DMODE_ST_PP_Y=2 [-DMODE_ST_PP_H=2 ...]     0 plain, 1 nt, 2 sc1, 3 sc0 sc1
# -> mode_diffusion_policy_amd/libmode_hip_<tag>.so (git-ignored); select it with MODE_HIP_LIB=<path>.  Only the translation units that read a
# redefined policy are recompiled; the shipped objects must be built first (make -C mode_diffusion_policy_amd/csrc).
set -e
TAG=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/mode_diffusion_policy_amd/csrc
T=${TMPDIR:-/tmp}/store_variant_$TAG; mkdir -p $T
declare -A USES=([MODE_ST_PP_H]="gemm_bf16_pp" [MODE_ST_PP_Y]="gemm_bf16_pp" [MODE_ST_PP_B]="gemm_bf16_pp" [MODE_ST_RING]="gemm_bf16" [MODE_ST_ATTN]="attn attn_long qkv_attn" [MODE_ST_ROW]="rowops")
TUS=""
for d in "$@"; do k=${d#-D}; k=${k%%=*}; TUS="$TUS ${USES[$k]}"; done
TUS=$(echo $TUS | tr ' ' '\n' | sort -u)
OBJS=""
for o in $C/*.o; do b=$(basename $o .o); echo "$TUS" | grep -qx "$b" || OBJS="$OBJS $o"; done
for tu in $TUS; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$R/include -I$C -Wno-unused-result "$@" -c $C/$tu.hip -o $T/$tu.o &
  OBJS="$OBJS $T/$tu.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS -o $R/mode_diffusion_policy_amd/libmode_hip_$TAG.so
echo built $R/mode_diffusion_policy_amd/libmode_hip_$TAG.so
