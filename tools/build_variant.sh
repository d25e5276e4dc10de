#!/bin/bash
# Dev tool: builds ONE kernel variant with arbitrary defines for A/B timing:
#   tools/build_variant.sh NAME [-DRTP_STATS] [-DRTP_WF_BLOCK=640 -DRTP_WF_MIN_WAVES=5] …
# → ray-tracing-practice_amd/variants/librtp_amd_NAME.so, used through RTP_AMD_LIB.
# The flags are the product's (`make print-render-flags`); a later flag on the line overrides one of them, so
#   tools/build_variant.sh slp -fslp-vectorize
# is the build WITH the SLP vectoriser for an A/B against the shipped flag set (docs/LOG.md round 24), and
#   DEV= tools/build_variant.sh nocarry -DRTP_DARK_CARRY=0
# the headline kernel without a radiance accumulator but also without the carried ray constants (round 32's A/B of the two steps;
# rt_timing.dark_kernel reports 2 for it).  The variant is a developer
# build without the tripwire (rt_debug_* entry points for RTP_STATS and the like); `DEV= tools/build_variant.sh NAME …` builds it
# exactly as the product's rt_capi.o is built.
set -e
cd "$(dirname "$0")/../ray-tracing-practice_amd" && mkdir -p variants
NAME=$1; shift
FLAGS="$(make -s print-render-flags) ${DEV--DRTP_DEV_BUILD -DRTP_TRIPWIRE=0}"
/opt/rocm/bin/hipcc $FLAGS "$@" -c -o variants/rt_capi_$NAME.o csrc/rt_capi.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/librtp_amd_$NAME.so variants/rt_capi_$NAME.o csrc/rt_accel.o csrc/rt_build.o csrc/rt_multi.o csrc/rt_denoise.o -ldl
echo "built variants/librtp_amd_$NAME.so"
