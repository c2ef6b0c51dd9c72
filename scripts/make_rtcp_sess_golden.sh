#!/bin/bash
# RTCP session goldens from the reference itself:
# scripts/gen_rtcp_sess_golden.c linked against the reference's
# src/rtp/pkt.c, rr.c, sdes.c, fb.c, member.c, source.c, rtp.c, ntp.c and
# src/hash/hash.c (plus the mbuf / mem / list / fmt / tmr / sa files they
# need to link), built into a temporary directory that is removed afterwards.
#   REF=/path/to/libre scripts/make_rtcp_sess_golden.sh
set -e -o pipefail
cd "$(dirname "$0")/.."
REF="${REF:-/root/reference}"
tmp="$(mktemp -d)"
trap 'rm -rf "$tmp"' EXIT
srcs=""
for f in src/rtp/pkt.c src/rtp/rr.c src/rtp/sdes.c src/rtp/fb.c \
         src/rtp/source.c src/rtp/member.c src/rtp/rtp.c src/rtp/ntp.c \
         src/hash/hash.c src/mbuf/mbuf.c src/mem/mem.c src/list/list.c \
         src/dbg/dbg.c src/fmt/print.c src/fmt/str.c src/fmt/str_error.c \
         src/tmr/tmr.c src/sa/sa.c; do
    srcs="$srcs $REF/$f"
done
${CC:-gcc} -O2 -ffunction-sections -fdata-sections -w \
    -DRELEASE -DHAVE_ATOMIC -DHAVE_PTHREAD -DHAVE_THREADS -DLINUX \
    -D_GNU_SOURCE -DHAVE_UNISTD_H -DHAVE_STRINGS_H -DHAVE_STRERROR_R \
    -I"$REF/include" -I"$REF/src/rtp" -Wall \
    -o "$tmp/gen_rtcp_sess_golden" scripts/gen_rtcp_sess_golden.c $srcs \
    -Wl,--gc-sections -lpthread
"$tmp/gen_rtcp_sess_golden" | gzip -9n > tests/golden/rtcp_sess_golden.json.gz
ls -la tests/golden/rtcp_sess_golden.json.gz
