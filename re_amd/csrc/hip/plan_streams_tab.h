/*
 * plan_streams_tab.h -- what the one-session planners share about the
 * session's stream table (plan_streams.hip builds it: k_sp_ssrc, k_sp_merge,
 * launched by sgpu_splan_table; plan_streams_rx.hip plans on it): the
 * geometry of those two launches and the slot of an SSRC in the table.
 */
#pragma once
#include "../srtpgpu.h"

#define SP_BLOCK 1024
#define SP_K SGPU_SP_MAX
#define SP_H 16                 /* per-block SSRC hash slots */

/* slot of SSRC s in the table (SP_K: none) */
__device__ __forceinline__ uint32_t sp_slot(const uint32_t *tab, uint32_t nt,
					    uint32_t s)
{
	uint32_t k = SP_K;
	for (uint32_t q = 0; q < nt; q++)
		if (tab[q] == s)
			k = q;
	return k;
}

static inline size_t sp_al(size_t x)
{
	return (x + 255) & ~(size_t)255;
}
