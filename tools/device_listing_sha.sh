#!/bin/bash
# SHA-256 of every translation unit's gfx950 device listing (the Makefile's CFLAGS plus --cuda-device-only -S), with the one token that depends on
# the host code (__hip_cuid_<hash>) replaced: two commits whose lines agree have byte-identical device code.
#   tools/device_listing_sha.sh [repository root, default: this one]      (compiles in place: kf_internal.h includes ../../include/hybkf.h)
set -euo pipefail
root=${1:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$root/hybkinectfu_amd/csrc"
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
cflags=$(make -pn 2>/dev/null | sed -n 's/^CFLAGS := //p' | head -1)
srcs=$(make -pn 2>/dev/null | sed -n 's/^SRCS := //p' | head -1)
pids=()
for f in $srcs; do
  ${HIPCC:-/opt/rocm/bin/hipcc} $cflags --cuda-device-only -S "$f" -o "$tmp/${f%.hip}.s" 2>"$tmp/${f%.hip}.err" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p" || { cat "$tmp"/*.err >&2; echo "a translation unit failed to compile" >&2; exit 1; }; done
for f in $srcs; do                                   # one line per SRCS entry, or the script fails
  printf '%s  %s\n' "$(sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$tmp/${f%.hip}.s" | sha256sum | cut -d' ' -f1)" "$f"
done | sort -k2
