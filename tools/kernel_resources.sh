#!/bin/bash
# Compiler's per-kernel resource usage (VGPR / SGPR / scratch / occupancy) of the shipped build (rt_capi.hip, then rt_denoise.hip) and,
# from the same cross-compile's assembly listing, each kernel's static instruction mix → profiles/<round>/kernel_resource_usage.txt
# (CPU only: hipcc cross-compiles for gfx950).  The flags are the Makefile's own (`make print-render-flags` / `print-hip-flags`).
#   tools/kernel_resources.sh r24 [extra compiler flags for rt_capi.hip, e.g. -fslp-vectorize, for a comparison listing]
# With extra flags the report goes to profiles/<round>/kernel_resource_usage_variant.txt instead.
set -eo pipefail
ROUND=${1:-r04}; shift || true
cd "$(dirname "$0")/../ray-tracing-practice_amd"
RENDERFLAGS="$(make -s print-render-flags) $*"
FLAGS="$(make -s print-hip-flags)"
OUT=../profiles/$ROUND/kernel_resource_usage.txt
[ $# -gt 0 ] && OUT=../profiles/$ROUND/kernel_resource_usage_variant.txt
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
# one device-only compile per translation unit: the remarks on stderr, the listing in the .s file
/opt/rocm/bin/hipcc $RENDERFLAGS -Rpass-analysis=kernel-resource-usage --cuda-device-only -S -o $TMP/rt_capi.s csrc/rt_capi.hip 2> $TMP/rt_capi_ru.txt
/opt/rocm/bin/hipcc $FLAGS -Rpass-analysis=kernel-resource-usage --cuda-device-only -S -o $TMP/rt_denoise.s csrc/rt_denoise.hip 2> $TMP/rt_denoise_ru.txt
mkdir -p ../profiles/$ROUND

# report LISTING REMARKS: the remark block of every kernel, followed by one line of static instruction counts of its listing.
#   VALU        every v_* instruction (v_nop excluded)
#   packed-fp32 v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 (half-rate pipe, docs/LOG.md §5g)
#   v_mov       v_mov_* and v_pk_mov_* (register shuffles; counted inside VALU too)
#   lane-moves  v_readlane / v_readfirstlane / v_writelane / v_permlane* / *_dpp / ds_bpermute / ds_permute / ds_swizzle
#   SALU        every s_* instruction except s_nop, s_waitcnt, s_load*/s_buffer_load* (memory), branches, barriers, s_endpgm, s_sleep;
#               "+ N other s_*" are those (SALU + N = every scalar-issued instruction but s_nop)
#   s_nop       hazard padding the compiler inserted (instructions, not the cycles they stand for)
report() {
  awk '
    FNR == NR {                                     # pass 1: the listing
      if ($0 ~ /^[A-Za-z_][A-Za-z0-9_$.]*:/) { fn = $1; sub(/:.*/, "", fn); seen[fn] = 1; next }
      if ($0 ~ /^\.Lfunc_end/) { fn = ""; next }
      if (fn == "" || $0 !~ /^\t[a-z]/) next
      op = $1
      if (op ~ /^v_/ && op != "v_nop") {
        valu[fn]++
        if (op ~ /^v_pk_(mul|add|fma)_f32/) pk[fn]++
        if (op ~ /^v_(pk_)?mov_/) mov[fn]++
      }
      if (op ~ /^v_(readlane|readfirstlane|writelane|permlane)/ || op ~ /_dpp$/ || $0 ~ /(quad_perm|row_shl|row_shr|row_ror|row_bcast|row_newbcast|row_mirror|row_half_mirror|wave_shl|wave_shr|wave_rol|wave_ror):?/ || op ~ /^ds_(bpermute|permute|swizzle)/) lane[fn]++
      if (op == "s_nop") nop[fn]++
      else if (op ~ /^s_/ && op !~ /^s_(waitcnt|load|buffer_load|branch|cbranch|barrier|endpgm|sleep|setprio|sethalt|trap|code_end|inst_prefetch|clause)/) salu[fn]++
      else if (op ~ /^s_/) sother[fn]++
      next
    }
    {                                               # pass 2: the remarks
      sub(/.*remark: /, ""); sub(/ \[-Rpass-analysis=kernel-resource-usage\]/, ""); sub(/^    /, "  ")
      if ($0 ~ /^Function Name: /) { cur = $3 }
      print
      if ($0 ~ /LDS Size/ && (cur in seen))
        printf "  Instructions: VALU %d, packed-fp32 %d, v_mov %d, lane-moves %d, SALU %d (+ %d other s_*), s_nop %d\n", valu[cur], pk[cur], mov[cur], lane[cur], salu[cur], sother[cur], nop[cur]
    }' "$1" <(grep -E "Function Name|TotalSGPRs|VGPRs:|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size" "$2") | c++filt
}
{
  echo "# hipcc $RENDERFLAGS -Rpass-analysis=kernel-resource-usage --cuda-device-only -S csrc/rt_capi.hip   ($(/opt/rocm/bin/hipcc --version | head -1))"
  echo "# render_kernel<kLds, kThreaded, kDyn, kWide, kSimple, kPrim>: <true,false,false,false,true,true> = the headline trace kernel (sphere-only build fed by the primary-visibility pass, for scenes without emitters: no radiance accumulator, the ray's sphere-test constants carried; -DRTP_DARK_CARRY=0 as an extra flag lists it without them), render_emit_kernel = the same walk carrying radiance (scenes with emitters, rt_config.dark_kernel = -1: the headline kernel's listing up to round 29), <false,false,true,true,false,true> = BASELINE configs[4] (distance-aware margins in parametric form on 4-wide nodes, records through L1/L2), <true,false,false,false,false,*> = the general octant kernel, <*,true,…> = the exact walks"
  echo "# Instructions: static counts of the kernel's listing (not executed counts): VALU = v_* without v_nop; packed-fp32 = v_pk_mul/add/fma_f32; v_mov = v_mov_* + v_pk_mov_* (inside VALU too); lane-moves = readlane/readfirstlane/writelane/permlane/DPP/ds_(b)permute/ds_swizzle; SALU = s_* without s_nop, s_waitcnt, memory loads, branches, barriers (those follow as \"other s_*\"); s_nop = hazard padding"
  report $TMP/rt_capi.s $TMP/rt_capi_ru.txt
  echo "# hipcc $FLAGS -Rpass-analysis=kernel-resource-usage --cuda-device-only -S csrc/rt_denoise.hip   (the denoiser's image-space kernels, rt_denoise)"
  report $TMP/rt_denoise.s $TMP/rt_denoise_ru.txt
} > $OUT
wc -l $OUT
