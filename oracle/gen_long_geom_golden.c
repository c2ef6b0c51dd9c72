/*
 * gen_long_geom_golden.c -- reference answers for SRTP and SRTCP packets of
 * about 2 KiB and above (TEST INFRASTRUCTURE ONLY).
 *
 * Linked against the reference libre sources compiled by oracle/Makefile
 * (target `ref`).  18 scenarios: every suite times {srtp_encrypt /
 * srtp_decrypt, srtcp_encrypt / srtcp_decrypt with flags 0, the same with
 * SRTP_UNENCRYPTED_SRTCP}.  In each
 *
 *   a sender protects one packet of every length L of the list below in turn
 *   (pos 0, ROOM spare bytes); a receiver with the same key and flags
 *   unprotects each protected packet right behind the sender's call, in a
 *   buffer with no room to spare.
 *
 * Lengths (plain packet bytes, ascending): every 37th from 208 to 1983, every
 * L in 1984..2112, then 4031, 4032, 4033 and 9000.
 *
 * A packet's bytes are a fixed function of (L, byte index i), restated by
 * tests/long_geom.py golden_packet(), so the file holds no inputs:
 *
 *   f(L, i) = (29 L + 7 i + 3 (i >> 4) + 1) mod 256
 *
 *   SRTCP: 81, 200 + L % 5, the 16-bit big-endian L / 4 - 1, the SSRC
 *          "lgeo", then f(L, i) for i >= 8.
 *   RTP:   f(L, i) everywhere but: byte 0 = 0x80 | X << 4 | CC, bytes 2-3 the
 *          sequence number (63450 + L) mod 65536 (it passes 65535 inside
 *          1984..2112), bytes 8-11 the SSRC, and with X set the extension
 *          header be de <words> behind the CSRCs.  The header is
 *          hl = 12 + 4 (L % 4) bytes (CC = L % 4: the four shift classes),
 *          and 76 + 4 (L % 4) bytes where L % 11 == 0 (CC = 15 and an
 *          extension of L % 4 words).
 *
 * Per call the file records the length, err, pos, end and size after the
 * call and the first 16 bytes of the SHA-256 of buf[0 : max(end before, end
 * after)); a receiver's input is the sender's output [0, end).  No
 * randomness, no time: two runs are identical.
 *
 * Usage: make -C oracle long_geom_golden
 *        (oracle/_ref/gen_long_geom_golden | gzip -9n >
 *         tests/golden/long_geom_golden.json.gz)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <openssl/sha.h>
#include <re.h>

#define SSRC   0x6c67656fu
#define LMAX   9000
#define ROOM   32               /* the sender's spare room: 4 + 16 at most */
#define SEQ0   63450

static const size_t keylen[6] = {30, 30, 46, 46, 28, 44};
static const char *kindname[3] = {"srtp", "srtcp", "srtcp_u"};

static void hexout(const uint8_t *p, size_t n)
{
	size_t i;
	putchar('"');
	for (i = 0; i < n; i++)
		printf("%02x", p[i]);
	putchar('"');
}

static void make_key(uint8_t *key, int suite, int kind)
{
	size_t i;
	for (i = 0; i < keylen[suite]; i++)
		key[i] = (uint8_t)(41 * i + 13 * suite + 7 * kind + 5);
}

static uint8_t f(size_t L, size_t i)
{
	return (uint8_t)(L * 29 + i * 7 + (i >> 4) * 3 + 1);
}

static void put_ssrc(uint8_t *p)
{
	p[0] = SSRC >> 24;
	p[1] = (SSRC >> 16) & 0xff;
	p[2] = (SSRC >> 8) & 0xff;
	p[3] = SSRC & 0xff;
}

static void build_rtcp(uint8_t *p, size_t L)
{
	const size_t words = L / 4 - 1;
	size_t i;
	for (i = 0; i < L; i++)
		p[i] = f(L, i);
	p[0] = 0x81;
	p[1] = (uint8_t)(200 + L % 5);
	p[2] = (uint8_t)(words >> 8);
	p[3] = (uint8_t)words;
	put_ssrc(p + 4);
}

static void build_rtp(uint8_t *p, size_t L)
{
	const unsigned seq = (unsigned)((SEQ0 + L) & 0xffff);
	const int ext = L % 11 == 0;
	const unsigned cc = ext ? 15 : (unsigned)(L % 4);
	size_t i;
	for (i = 0; i < L; i++)
		p[i] = f(L, i);
	p[0] = (uint8_t)(0x80 | (ext ? 0x10 : 0) | cc);
	p[2] = (uint8_t)(seq >> 8);
	p[3] = (uint8_t)seq;
	put_ssrc(p + 8);
	if (ext) {
		uint8_t *x = p + 12 + 4 * cc;
		x[0] = 0xbe;
		x[1] = 0xde;
		x[2] = 0;
		x[3] = (uint8_t)(L % 4);
	}
}

static int first_call;

/* one reference call on a fresh mbuf of `size` bytes holding in[0:end) at pos
 * 0, zero behind; out receives max(end, end after) bytes.  Returns the end
 * after. */
static size_t run_op(struct srtp *s, int rtcp, int dec, size_t L,
		     const uint8_t *in, size_t size, size_t end, uint8_t *out)
{
	struct mbuf *mb = mbuf_alloc(size);
	uint8_t md[SHA256_DIGEST_LENGTH];
	size_t rec, e;
	int err;

	memset(mb->buf, 0, mb->size);
	memcpy(mb->buf, in, end);
	mb->pos = 0;
	mb->end = end;
	if (rtcp)
		err = dec ? srtcp_decrypt(s, mb) : srtcp_encrypt(s, mb);
	else
		err = dec ? srtp_decrypt(s, mb) : srtp_encrypt(s, mb);
	rec = mb->end > end ? mb->end : end;
	SHA256(mb->buf, rec, md);
	printf("%s\n [%zu,%d,%zu,%zu,%d,%zu,%zu,%zu,", first_call ? "" : ",", L,
	       dec, size, end, err, mb->pos, mb->end, mb->size);
	first_call = 0;
	hexout(md, 16);
	printf("]");
	memcpy(out, mb->buf, rec);
	e = mb->end;
	if (err) {
		fprintf(stderr, "L %zu dec %d: err %d\n", L, dec, err);
		exit(1);
	}
	mem_deref(mb);
	return e;
}

static size_t lens[256];
static size_t nlens;

static void scenario(int suite, int kind, int first)
{
	static uint8_t pkt[LMAX], prot[LMAX + ROOM], out[LMAX + ROOM];
	const int flags = kind == 2 ? SRTP_UNENCRYPTED_SRTCP : 0;
	uint8_t key[64];
	struct srtp *tx = NULL, *rx = NULL;
	size_t k;

	make_key(key, suite, kind);
	if (srtp_alloc(&tx, suite, key, keylen[suite], flags) ||
	    srtp_alloc(&rx, suite, key, keylen[suite], flags)) {
		fprintf(stderr, "srtp_alloc failed\n");
		exit(1);
	}
	printf("%s\n{\"name\":\"long_geom_%s_s%d\",\"kind\":\"%s\",\"suite\":%d,"
	       "\"flags\":%d,\"key\":", first ? "" : ",", kindname[kind], suite,
	       kind ? "srtcp" : "srtp", suite, flags);
	hexout(key, keylen[suite]);
	printf(",\"calls\":[");
	first_call = 1;
	for (k = 0; k < nlens; k++) {
		const size_t L = lens[k];
		size_t n;
		if (kind)
			build_rtcp(pkt, L);
		else
			build_rtp(pkt, L);
		n = run_op(tx, kind != 0, 0, L, pkt, L + ROOM, L, prot);
		run_op(rx, kind != 0, 1, L, prot, n, n, out);
	}
	printf("]}");
	mem_deref(tx);
	mem_deref(rx);
}

int main(void)
{
	size_t L, k;
	int s, kind;

	for (L = 208; L < 1984; L += 37)
		lens[nlens++] = L;
	for (L = 1984; L <= 2112; L++)
		lens[nlens++] = L;
	lens[nlens++] = 4031;
	lens[nlens++] = 4032;
	lens[nlens++] = 4033;
	lens[nlens++] = 9000;

	printf("{\"generator\":\"oracle/gen_long_geom_golden.c\","
	       "\"columns\":[\"L\",\"dec\",\"size\",\"end\",\"err\",\"pos_o\","
	       "\"end_o\",\"size_o\",\"sha256_16\"],\"seq0\":%d,\"ssrc\":%u,"
	       "\"room\":%d,\"lengths\":[", SEQ0, SSRC, ROOM);
	for (k = 0; k < nlens; k++)
		printf("%s%zu", k ? "," : "", lens[k]);
	printf("],\"scenarios\":[");
	for (s = 0; s < 6; s++)
		for (kind = 0; kind < 3; kind++)
			scenario(s, kind, s == 0 && kind == 0);
	printf("\n]}\n");
	return 0;
}
