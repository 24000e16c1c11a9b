// fseq_path_setup.hip -- the segmentation path, what a run stands on: pinned host staging, the alignment's memory, the block
// geometry and the kernel choice, the work buffers, the row upload, and the one exchange primitive of a sharded run.
// (The units of the path and what crosses them: fseq_path.hpp.)
#include "fseq_path.hpp"
#include "fseq_kernels.hpp"
#include "fseq_dp.hpp"           // dp_schedule (the halo of a sharded rank)
#include "fseq_stream.hpp"       // the sizes of the streamed kernels' LDS, workspaces and stride states
#include "fseq_blockkeys.hpp"    // ... and of phase A in key space
#include "fseq_chainplan.hpp"    // the fan of phase B and a sharded rank's (k, q)

namespace fseq {

int pin_reserve(fseq_ctx *c, size_t bytes)
{
	c->pin_used = 0;
	if (c->pin_cap >= bytes) return FSEQ_OK;
	if (c->h_pin) (void) hipHostFree(c->h_pin);
	c->h_pin = nullptr; c->pin_cap = 0;
	size_t const cap = std::max<size_t>((bytes + 4095) & ~size_t(4095), size_t(1) << 20);
	hipError_t const e = hipHostMalloc(reinterpret_cast<void **>(&c->h_pin), cap, hipHostMallocDefault);
	if (e != hipSuccess) { c->h_pin = nullptr; return fail(c, FSEQ_E_OOM, "hipHostMalloc of the staging buffer", e); }
	c->pin_cap = cap;
	return FSEQ_OK;
}

void free_msa(fseq_ctx *c)
{
	c->d_msa_own.release(c);
	c->d_msa = nullptr;
	c->have_input = false;
	if (c->in.open) c->free_input();         // (a chunked input under way ends where another input takes its place)
}

int alloc_msa(fseq_ctx *c)
{
	free_msa(c);
	c->bsh = c->sigma <= 4 ? 2u : c->sigma <= 16 ? 1u : 0u;
	c->ld = ((size_t) sym_bytes(c->p.m, c->bsh) + 15) & ~size_t(15);
	int rc = c->d_msa_own.alloc(c, c->ld * (held_hi(c) - held_lo(c)) + 16);
	if (rc) return rc;
	c->d_msa = c->d_msa_own.base - held_lo(c) * c->ld;       // column k at d_msa + k * ld for the held columns
	return FSEQ_OK;
}

// Block structure of phases A-C.  Sharded: every rank is one hyper-block of phase B (shard_q groups of
// chain_fan^shard_k blocks), so the only exchange of phase B is the W composite key blocks of the ranks.
void block_geometry(fseq_ctx *c)
{
	fseq_params const &p = c->p;
	bool const streamed = p.m > 11264u;
	Shard &sh = c->sh;
	if (p.block_len) c->B = p.block_len;
	else if (c->auto_B) c->B = c->auto_B;                    // (prepare_geometry's second look, below)
	else if (!sh.on)
	{
		// LDS-resident kernels: ~1024 blocks (2-4 workgroups per CU).  Streamed kernels stage a whole column
		// in LDS (one workgroup per CU) and pay the phase-B chain per block and per row: ~256 blocks.
		// (32-bit LDS state and long inputs: ~4096 blocks -- measured on BASELINE C3: phase C 7.7 -> 7.3 ms with the finer
		// grain, phase B 0.50 -> 0.74 ms with its two more levels; blocks of fewer than ~200 columns lose more to the
		// per-block prologues and to phase B than they gain)
		uint64_t target = streamed ? 256u : 1024u;
		if (!streamed && p.m <= 7168u && p.n >= 4096u * 200u) target = 4096u;
		uint64_t b = (p.n + target - 1) / target;
		if (b < 16) b = 16;
		if (b > 4096) b = 4096;
		c->B = (uint32_t) b;
	}
	else
	{
		// sharded: the same per rank, and -- streamed kernels are one workgroup per CU -- a whole number of waves of
		// workgroups per rank (256 CUs x k blocks of <= 4096 columns), so that no rank ends on a nearly empty wave
		int ncu = 0;
		(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p.device);
		if (ncu < 1) ncu = 256;
		uint64_t const cols = (p.n + sh.world - 1) / sh.world;
		// (streamed rows: blocks of ~1,600 columns, see prepare_geometry)
		uint64_t const per_cu_cols = streamed ? STREAM_BLOCK_TARGET : 4096u;
		uint64_t k = std::max<uint64_t>(1, (cols + (uint64_t) ncu * per_cu_cols / 2) / ((uint64_t) ncu * per_cu_cols));
		// (the second form of the streamed phase C runs -- and was tuned for -- two workgroups per CU: a rank's blocks are whole
		// rounds of 2 x CUs workgroups, also when one workgroup per CU would hold its columns: BASELINE C4 on 8 ranks is 512
		// blocks of 1,221 columns per rank, not 256 of 2,442 with every CU's second slot empty)
		if ((k & 1u) && (uint64_t) p.m + 4096u < (1ull << 19) && !c->tune.stream_plain_scan) ++k;
		uint64_t per = streamed ? (uint64_t) ncu * k : 1024u;
		uint64_t b = (p.n + per * sh.world - 1) / (per * sh.world);
		if (b < 16) b = 16;
		c->B = (uint32_t) b;
	}
	// sharded: the DP round that starts on a rank's last column reads the lists of the RL - 1 columns behind it; the
	// rank produces them itself by running into the next rank's first block -- which must hold them: B >= RL
	uint32_t halo = 0;
	if (sh.on && p.n >= 2 * p.segment_length)
	{
		halo = dp_schedule((uint32_t) p.segment_length, (uint32_t) p.n).RL;
		if (c->B < halo) c->B = halo;
	}
	if (c->B > p.n) c->B = (uint32_t) p.n;
	c->nblocks = (uint32_t) ((p.n + c->B - 1) / c->B);
	if (sh.on)
	{
		// A rank is one hyper-block of phase B: q groups of F^k blocks, composed level by level with fan F; (k, q) with the fewest
		// serial steps among those that keep every rank busy (plan_chain_sharded, fseq_chainplan.hpp)
		ShardChainPlan const S = plan_chain_sharded(c->nblocks, sh.world, c->tune.chain_fan ? (uint32_t) c->tune.chain_fan : CHAIN_SHARD_FAN);
		c->chain_fan = S.F; c->shard_k = S.k; c->shard_q = S.q;
		sh.bpr = S.bpr;
		c->chain_G = S.group; c->chain_G2 = S.q;                   // (diagnostics: a rank = chain_G2 groups of chain_G blocks)
		c->n_super = S.n_super;
		c->n_hyper = S.n_hyper;
		sh.active = c->n_hyper;                                 // <= world
		sh.b_lo = std::min<uint64_t>(c->nblocks, (uint64_t) sh.rank * sh.bpr);
		sh.b_hi = std::min<uint64_t>(c->nblocks, (uint64_t) (sh.rank + 1) * sh.bpr);
		sh.c_lo = std::min<uint64_t>(p.n, (uint64_t) sh.b_lo * c->B);
		sh.c_hi = std::min<uint64_t>(p.n, (uint64_t) sh.b_hi * c->B);
		sh.c_end = (sh.b_hi > sh.b_lo) ? std::min<uint64_t>(p.n, sh.c_hi + halo) : sh.c_hi;
		return;
	}
	{
		// Phase B is serial over key blocks, so it is applied recursively: compose groups of G blocks from the identity (parallel),
		// groups of G of those, ... until at most G are left, chain them, expand level by level.  The fan G is plan_chain_fan's
		// (fseq_chainplan.hpp): by the serial depth on LDS-resident rows, by round 5's cost model on streamed rows, and [r14] among the
		// wider fans by turns of workgroups where level 0 has at least a chain per CU and goes to k_chain_wg (launch_chain,
		// fseq_path_pass1.hip).
		// BASELINE C4 (6,143 blocks, 100,000 rows), phase B by round 5's kernels: fan 3: 69.6 ms, 4: 61.6, 6: 56.5, 8: 54.1, 12: 50.9, 16: 53.7,
		// 32: 57.5.  With level 0 on k_chain_wg (measured: a step 0.5 ms by runs, 0.8 by the sort of the rows, 0.9 from the identity; the
		// step is bound by the bytes it moves, which go with the rows): fan 11 (round 5's; 559 chains, 3 turns) 43.0 ms, 12 (512, 2 turns)
		// 38.0, 24 (256, one turn) 36.8 -- the model's order.  Every other shape on one GPU keeps round 5's fan: with fewer than CUs x fan
		// blocks (C4slice, C4cols50k) no level reaches the kernel.  FSEQ_CHAIN_WG=1 or 2 (tests): round 5's fan.
		KernelSet probe;
		bool const stream_model = !select_kernels(p.m, c->sigma, &probe);
		uint32_t const best_g = plan_chain_fan(p.m, stream_model, c->nblocks, stream_model && c->tune.chain_wg == 0 && c->nblocks > 8 ? device_cus(c) : 0, c->tune.chain_wg,
		                                       (uint32_t) c->tune.chain_fan).fan;
		c->chain_fan = best_g;
		c->chain_G = best_g; c->n_super = (c->nblocks + best_g - 1) / best_g;      // (diagnostics)
		c->chain_G2 = 0; c->n_hyper = 0;
	}
}

int prepare_geometry(fseq_ctx *c)
{
	fseq_params const &p = c->p;
	c->auto_B = 0;
	block_geometry(c);
	uint32_t n2 = 1;
	while (n2 < p.m) n2 <<= 1;
	if (n2 < 2) n2 = 2;
	c->N2 = n2;
	{
		uint32_t bits = 1;
		while ((1u << bits) < c->sigma) ++bits;
		c->npass = (bits + 1) / 2;               // 2-bit digit passes per column
	}
	if (c->sigma > 256) return fail(c, FSEQ_E_UNSUPPORTED, "alphabet larger than 256 symbols");
	c->use_stream = !select_kernels(p.m, c->sigma, &c->ks);
	if (c->use_stream)
	{
		// rows beyond the LDS-resident configurations: the order streams through HBM / L2
		if (sym_bytes(p.m, c->bsh) > STREAM_MAX_COLBYTES)
			return fail(c, FSEQ_E_UNSUPPORTED, "more rows than this build handles (one packed column must fit LDS: 147456 bytes)");
		// the tile staging buffer of stream_pass (64 KiB) when the staged column leaves room for it
		c->stream_staged = stream_lds_bytes(sym_bytes(p.m, c->bsh), true) <= LDS_LIMIT;
		size_t const lds = stream_lds_bytes(sym_bytes(p.m, c->bsh), c->stream_staged);
		if (int const rc = prepare_stream_kernels(c, lds)) return rc;
		// phase C in its second form (fseq_stream2.hpp) while every value id (< m + B) fits the key shift of its tile and the
		// column is staged (FSEQ_STREAM_PLAIN_SCAN keeps the first form)
		c->s2 = Stream2Config{};
		{
			Stream2Config const cfg = stream2_config();
			if (!c->tune.stream_plain_scan && (uint64_t) p.m + c->B < (1ull << cfg.key_shift) && c->stream_staged)
			{
				size_t const bytes = cfg.lds(sym_bytes(p.m, c->bsh));
				if (bytes <= LDS_LIMIT)
				{
					HIP_TRY(c, cfg.prepare(bytes));
					if (int const rc = prepare_stream2_prologue(c)) return rc;
					c->s2 = cfg; c->s2_lds = bytes;
				}
			}
		}
		// Long inputs (the block length was clamped to 4,096 columns): whole rounds of phase C's workgroups.  BASELINE C4 had
		// 1,221 blocks on 512 slots -- 2.4 rounds, the last one 38 % full: 2.33 s; 1,536 blocks of 3,256 columns: 2.22 s
		// (2,048 and 3,072 blocks the same: phase A gains what phase B loses).
		// [r4] ... and blocks of ~1,600 columns: the streamed key-space tree is cheaper per column in shorter blocks (its merges with
		// the running prefix see fewer distinct keys), and phase B no longer pays for more blocks what it did (fseq_chainsort.hpp).
		// BASELINE C4, blocks x columns: 1,536 x 3,256: A 340 + B 32 = 1,823 ms the step; 2,048 x 2,442: 317 + 41 = 1,823;
		// 3,072 x 1,628: 280 + 50 = 1,791; 4,096 x 1,221: 263 + 64 = 1,793.
		if (!p.block_len && !c->sh.on && !c->auto_B && c->B > STREAM_BLOCK_TARGET && c->B < p.n)
		{
			int ncu = 0;
			(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p.device);
			uint64_t const slots = (uint64_t) std::max(ncu, 1) * (c->s2.T ? c->s2.resident(c->s2_lds) : 1u);
			uint64_t const rounds = std::max<uint64_t>(1, (p.n + slots * STREAM_BLOCK_TARGET / 2) / (slots * STREAM_BLOCK_TARGET));
			uint64_t const b = (p.n + rounds * slots - 1) / (rounds * slots);
			if (c->tune.debug) fprintf(stderr, "[fseq] streamed phase C: %u blocks on %llu workgroup slots -> %llu rounds of %llu columns\n", c->nblocks, (unsigned long long) slots,
			                           (unsigned long long) rounds, (unsigned long long) b);
			if (b >= 256 && b < c->B)
			{
				c->auto_B = (uint32_t) b;
				block_geometry(c);
			}
		}
		// phase A in key space, streamed rows: the bitmap (and its 32-bit prefix counts) take the LDS
		c->bk_cap_words = 12288;                               // two bitmaps + 32-bit prefix counts: 12 B per word
		if (c->tune.blockkeys_cap) c->bk_cap_words = (uint32_t) c->tune.blockkeys_cap;
		c->bk_lds = blockkeys_stream_lds_bytes(c->bk_cap_words, 1024);
		// (bk_merge slices a merge by whole `hi` values: one hi value's Dlo <= m keys must fit the bitmap -- with more rows
		// than bitmap bits a diverse block could overrun it, so such inputs take the column sweep k_colblock_stream<MODE_RANK>)
		if (c->bk_lds <= LDS_LIMIT && (uint64_t) p.m <= (uint64_t) c->bk_cap_words * 32u)
		{
			if (int const rc = prepare_blockkeys_stream(c)) return rc;
		}
		else c->bk_cap_words = 0;
	}
	else
	{
		c->lds_columns = c->ks.columns_lds(c->B);
		if (c->lds_columns > LDS_LIMIT || c->ks.lds_chain > LDS_LIMIT || c->ks.lds_colblock > LDS_LIMIT || c->ks.lds_snap > LDS_LIMIT)
			return fail(c, FSEQ_E_UNSUPPORTED, "block state does not fit the 160 KiB LDS of one CU");
		// phase C works on value ids < m + B in 16-bit keys (partition_step<.., KEY16>); the LDS check above implies it
		if ((uint64_t) p.m + c->B > 65535u) return fail(c, FSEQ_E_UNSUPPORTED, "block length too large for the 16-bit value ids of phase C");
		HIP_TRY(c, c->ks.prepare());
		HIP_TRY(c, c->ks.prepare_columns(c->lds_columns));
		// Short inputs: phase C is a few rounds of (CUs x workgroups per CU) blocks, and a last round that is a third full
		// costs a whole one (BASELINE C2: 1,021 blocks on 768 slots; 764 blocks of 131 columns: phase C 0.65 -> 0.59 ms).
		// Below three rounds the block length is refitted to whole rounds (long inputs measured no better for it).
		if (!p.block_len && !c->sh.on && !c->auto_B)
		{
			int ncu = 0;
			(void) hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p.device);
			uint64_t const slots = (uint64_t) std::max(ncu, 1) * c->ks.columns_resident(c->lds_columns);
			if (c->tune.debug) fprintf(stderr, "[fseq] phase C: %u blocks of %u columns on %llu workgroup slots (%zu bytes of LDS each)\n", c->nblocks, c->B, (unsigned long long) slots, c->lds_columns);
			if (c->nblocks > slots && c->nblocks < 3 * slots)
			{
				uint64_t const rounds = (c->nblocks + slots / 2) / slots;
				uint64_t const b = (p.n + rounds * slots - 1) / (rounds * slots);
				if (b >= 16 && b <= 4096 && b != c->B && p.m + b <= 65535u)
				{
					c->auto_B = (uint32_t) b;
					block_geometry(c);
					c->lds_columns = c->ks.columns_lds(c->B);
					// (rounds is rounded down, so the refit can RAISE the block length by up to ~1.5x: when the longer block no
					// longer fits the LDS, or holds another number of workgroups per CU than it was fitted for, keep the first one)
					if (c->lds_columns > LDS_LIMIT || (uint64_t) std::max(ncu, 1) * c->ks.columns_resident(c->lds_columns) != slots)
					{
						c->auto_B = 0;
						block_geometry(c);
						c->lds_columns = c->ks.columns_lds(c->B);
					}
					HIP_TRY(c, c->ks.prepare_columns(c->lds_columns));
				}
			}
		}
		// phase A in key space: the id arrays are (GL + 2) x m halfwords; the two maps take what is left of ~76 KiB
		// (two workgroups per CU) when that holds the leaf map with a quarter to spare, else of the whole CU
		{
			c->bk_T = blockkeys_threads(p.m);
			size_t const arrays = blockkeys_lds_bytes(p.m, 0, (int) c->bk_T, c->ld, c->bsh);
			size_t budget = 76 * 1024;
			if (arrays + 16 * 2560 > budget) budget = LDS_LIMIT - 1024;
			size_t cap = budget > arrays ? (budget - arrays) / 16 : 0;     // two maps of 8-byte {bits, prefix} entries
			cap = std::min<size_t>(cap & ~size_t(63), 32768);
			if (c->tune.blockkeys_cap) cap = (size_t) c->tune.blockkeys_cap;     // tests: force the sliced merges
			c->bk_cap_words = (uint32_t) cap;
			c->bk_lds = blockkeys_lds_bytes(p.m, c->bk_cap_words, (int) c->bk_T, c->ld, c->bsh);
			// (a leaf's columns are staged with two 16-byte pieces per thread)
			if (cap >= 2048 && c->bk_lds <= LDS_LIMIT && (size_t) (8u >> (2u - c->bsh)) * c->ld <= (size_t) c->bk_T * 32) HIP_TRY(c, prepare_blockkeys(c->bk_T, c->bk_lds, c->tune.debug));
			else c->bk_cap_words = 0;
		}
	}
	if (int const rc = prepare_dp_kernels(c)) return rc;
	c->kernels_ready = true;
	return FSEQ_OK;
}

namespace {

void release_levels(fseq_ctx *c)
{
	for (auto &lv : c->levels) release_all(c, lv.rank, lv.keyd, lv.nkeys, lv.state_a, lv.state_d);
	c->levels.clear();
}

// the buffers whose sizes follow from the geometry alone: per column block, per column, per DP entry
int alloc_geometry_buffers(fseq_ctx *c)
{
	fseq_params const &p = c->p;
	size_t const m = p.m;
	int rc;
	// my blocks [bl, bh) (all of them when not sharded); boundary states also behind my last block
	size_t const bl = c->sh.on ? c->sh.b_lo : 0, bh = c->sh.on ? std::max(c->sh.b_hi, c->sh.b_lo) : c->nblocks;
	if ((rc = c->d_rank.alloc_range(c, bl, bh, m))) return rc;
	if ((rc = c->d_keyd.alloc_range(c, bl, bh, m))) return rc;
	if ((rc = c->d_nkeys.alloc_range(c, bl, bh, 1))) return rc;
	if ((rc = c->d_bstate_a.alloc_range(c, bl, bh + 1, m))) return rc;
	if ((rc = c->d_bstate_d.alloc_range(c, bl, bh + 1, m))) return rc;
	{
		// the composites of phase B, level by level: until at most chain_fan are left, or -- sharded -- shard_k levels below
		// the hyper key blocks (indexed like the blocks: by their place in the whole alignment; a rank holds its own range)
		// (the items of the levels on one GPU: chain_level_items, fseq_chainplan.hpp -- the plan the tests read)
		std::vector<uint32_t> const items = c->sh.on ? std::vector<uint32_t>() : chain_level_items(c->nblocks, c->chain_fan);
		uint32_t cnt = c->nblocks;
		uint64_t cols = c->B;
		size_t lo = bl, hi = bh;
		for (uint32_t i = 0; c->sh.on ? i < c->shard_k : i + 1 < items.size(); ++i)
		{
			fseq_ctx::ChainLevel lv;
			lv.count = c->sh.on ? (cnt + c->chain_fan - 1) / c->chain_fan : items[i + 1];
			lv.cols = cols * c->chain_fan;
			lo = lo / c->chain_fan; hi = (hi + c->chain_fan - 1) / c->chain_fan;
			c->levels.push_back(lv);                               // (pushed at once: release_levels releases what is there)
			fseq_ctx::ChainLevel &L = c->levels.back();
			if ((rc = L.rank.alloc_range(c, lo, hi, m))) return rc;
			if ((rc = L.keyd.alloc_range(c, lo, hi, m))) return rc;
			if ((rc = L.nkeys.alloc_range(c, lo, hi, 1))) return rc;
			if ((rc = L.state_a.alloc_range(c, lo, hi + 1, m))) return rc;
			if ((rc = L.state_d.alloc_range(c, lo, hi + 1, m))) return rc;
			cnt = L.count; cols = L.cols;
		}
	}
	if (c->sh.on && c->n_hyper)
	{
		if ((rc = c->d_hrank.alloc(c, (size_t) c->n_hyper * m))) return rc;
		if ((rc = c->d_hkeyd.alloc(c, (size_t) c->n_hyper * m))) return rc;
		if ((rc = c->d_hnkeys.alloc(c, c->n_hyper))) return rc;
		if ((rc = c->d_hstate_a.alloc(c, ((size_t) c->n_hyper + 1) * m))) return rc;
		if ((rc = c->d_hstate_d.alloc(c, ((size_t) c->n_hyper + 1) * m))) return rc;
	}
	if ((rc = c->d_hdr.alloc(c, p.n))) return rc;
	if ((rc = c->d_flags.alloc(c, 1))) return rc;
	if ((rc = c->d_recent.alloc(c, c->nblocks + 1))) return rc;
	if (p.n >= 2 * p.segment_length)
	{
		c->dp_size = p.n - p.segment_length + 1;
		c->dp.tstride = (uint32_t) (c->dp_size / 64 + 2);
		if ((rc = c->dp.M.alloc(c, c->dp_size))) return rc;
		if ((rc = c->dp.LB.alloc(c, c->dp_size))) return rc;
		if ((rc = c->dp.SZ.alloc(c, c->dp_size))) return rc;
		if ((rc = c->dp.K.alloc(c, c->dp_size + 64))) return rc;
		if ((rc = c->dp.Tb.alloc(c, (size_t) 32 * c->dp.tstride))) return rc;
		if ((rc = c->dp.Tbv.alloc(c, (size_t) 32 * c->dp.tstride))) return rc;
		if ((rc = c->d_Mprev.alloc(c, c->dp_size))) return rc;
	}
	return FSEQ_OK;
}

} // namespace

int ensure_work_buffers(fseq_ctx *c, uint32_t X, bool want_ss)
{
	fseq_params const &p = c->p;
	size_t const m = p.m;
	int rc;
	if (!c->d_rank && (rc = alloc_geometry_buffers(c)))
	{
		// (all of them or none: d_rank stands for the rest, and the levels are pushed as they are allocated)
		release_levels(c);
		c->d_rank.release(c);
		return rc;
	}
	if (c->use_stream && !c->d_ws)
	{
		// one workspace per block of phase C (sharded: my blocks and the halo block behind them); phase A's column sweep, phase B
		// and pass 2 index the same memory by workgroup (4m words each)
		size_t const per_block = std::max<size_t>(columns_stream_ws_words(p.m, c->B), (size_t) 4 * m);
		size_t const bl = c->sh.on ? c->sh.b_lo : 0, bh = c->sh.on ? std::min<size_t>(c->nblocks, (size_t) std::max(c->sh.b_hi, c->sh.b_lo) + 1) : c->nblocks;
		if ((rc = c->d_ws.alloc(c, per_block * std::max<size_t>(bh - bl, 1)))) return rc;
		c->d_ws.rebase((ptrdiff_t) (bl * columns_stream_ws_words(p.m, c->B)));
		// phase B spread over the chip: the digit histograms of every part of every chain of a launch (the widest launch of the
		// recursion has a chain per chain_fan blocks; a sharded rank's own range the same)
		// (streamed rows are < 2^20: one packed column fits STREAM_MAX_COLBYTES, so m <= 4 x 147,456 = 589,824)
		size_t const chains = std::max<size_t>(1, (bh - bl + std::max(2u, c->chain_fan) - 1) / std::max(2u, c->chain_fan) + 1);
		if ((rc = c->d_cshist.alloc(c, chains * chain_hist_words(p.m)))) { c->d_ws.release(c); return rc; }
	}
	uint64_t const k_lo = held_lo(c), k_cnt = held_hi(c) - k_lo;      // sharded: lists and stride states of my columns only
	// (a list budget: the H + wb B columns of one window, plan_list_windows)
	size_t const ent_count = c->lw.on ? ((size_t) c->lw.H + (size_t) c->lw.wb * c->B) * ((X + 3) & ~1u) + 256 : (size_t) k_cnt * ((X + 3) & ~1u) + 256;
	if (X && (!c->d_ent || c->X != X || c->d_ent.cap != ent_count))
	{
		c->X = X;
		c->stride = (X + 3) & ~1u;                // lump + up to X+1 entries, even
		rc = c->d_ent.alloc(c, ent_count);        // padded: the DP loads strips unconditionally
		if (rc == FSEQ_E_OOM && c->d_ss_a)
		{
			// the stride states were sized before the lists grew: give their memory back and size them again below
			release_all(c, c->d_ss_a, c->d_ss_d);
			rc = c->d_ent.alloc(c, ent_count);
		}
		if (rc) return rc;
		c->d_ent.rebase((ptrdiff_t) ((size_t) k_lo * c->stride));   // list of column k at d_ent + k * stride (windows: set per window)
	}
	if (X && want_ss && !c->d_ss_a && p.n >= 2 * p.segment_length)
	{
		// stride states for pass 2: one (a, d) pair of m words each every snap_stride columns.  Sized after the lists:
		// what is free now, minus the boundary snapshots pass 2 will need at most (one per L columns) and a margin,
		// within [4 GiB, 160 GiB]; the smallest stride >= 16 (8: below) that fits.  (FSEQ_DEBUG prints the choice.)
		// streamed rows: 5 bytes per row when a row id and a column number fit 40 bits together (fseq_stream.hpp)
		c->ss_pack = 0;
		c->ss_ids = false;
		if (c->use_stream && !c->tune.ss_unpacked)
		{
			uint32_t abits = 1, dbits = 1;
			while ((1ull << abits) < m) ++abits;
			while ((1ull << dbits) <= p.n) ++dbits;
			if (abits + dbits <= 40 && abits < 32) c->ss_pack = abits;
			// second form of the streamed phase C on packed rows: the states in id form (its packed rows as they are: a row id and
			// a value id below 2^19 always fit 40 bits), pass 2 on the same tile step
			if (c->s2.T && !c->tune.ss_absolute) { c->ss_pack = abits; c->ss_ids = true; }
		}
		if (c->ss_ids && !c->d_bs_w)
		{
			// every block's start state in id form (written by the prologue of phase C): my blocks and the halo block
			size_t const bl = c->sh.on ? c->sh.b_lo : 0, bh = c->sh.on ? std::min<size_t>(c->nblocks, (size_t) std::max(c->sh.b_hi, c->sh.b_lo) + 1) : c->nblocks;
			if ((rc = c->d_bs_w.alloc_range(c, bl, std::max(bh, bl + 1), m))) return rc;
			if ((rc = c->d_bs_h.alloc_range(c, bl, std::max(bh, bl + 1), ss_high_stride(p.m)))) { c->d_bs_w.release(c); return rc; }
		}
		uint64_t budget = 4ull << 30;
		{
			size_t free_b = 0, total_b = 0;
			if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
			{
				// (everything else of any size is allocated by now: the margin covers the traceback / task arrays of the
				// tail, a few MB, and fragmentation -- BASELINE C4 on one GPU sits within 1 GiB of the 64-column stride)
				uint64_t const reserve = (k_cnt / p.segment_length + 1) * (uint64_t) m * 8ull + (2ull << 30);
				// (a context with a memory budget -- ranks that share a card -- plans inside what is left of it)
				uint64_t mine = free_b;
				if (c->mem_budget) mine = std::min<uint64_t>(mine, c->mem_budget > c->alloc_total ? c->mem_budget - c->alloc_total : 0);
				uint64_t const avail = mine > reserve ? mine - reserve : 0;
				budget = std::max<uint64_t>(budget, std::min<uint64_t>(avail, 160ull << 30));
			}
		}
		uint64_t const state_bytes = c->ss_pack ? (uint64_t) m * 4ull + ss_high_stride(p.m) : (uint64_t) m * 8ull;
		// first stride tried: 16 columns; 8 where a column is two digit passes (pass 2 replays stride / 2 columns per boundary at
		// twice the price there, a state costs phase C the same: BASELINE C5 pass 2 4.3 -> 2.3 ms, phase C 36.7 -> 36.9;
		// sigma <= 4: BASELINE C3 8.7 / 8.6 / 8.6 / 8.7 ms for 8 / 12 / 16 / 24)
		uint64_t st_ = (c->npass >= 2 && !c->use_stream) ? 8 : 16;
		// the smallest stride >= 16 whose states fit (any number, not a power of two: pass 2 costs ~stride / 2 columns per boundary)
		if ((k_cnt / st_ + 2) * state_bytes > budget) st_ = std::max<uint64_t>(st_, (k_cnt * state_bytes + budget - 1) / std::max<uint64_t>(1, budget - 2 * state_bytes));
		while ((k_cnt / st_ + 2) * state_bytes > budget) ++st_;
		c->snap_stride = (uint32_t) st_;
		if (c->tune.debug) fprintf(stderr, "[fseq] stride states every %llu columns (budget %.1f GiB, %llu bytes per state)\n", (unsigned long long) st_, budget / 1073741824.0, (unsigned long long) state_bytes);
		uint64_t const q_lo = k_lo / st_, q_hi = held_hi(c) / st_;
		// state at column q * snap_stride at d_ss_* + q * m (packed: the high bytes at d_ss_d + q * hs BYTES)
		size_t const hs = ss_high_stride(p.m);
		if ((rc = c->d_ss_a.alloc_range(c, q_lo, q_hi + 1, m))) return rc;
		if (c->ss_pack) { rc = c->d_ss_d.alloc(c, ((size_t) (q_hi - q_lo + 1) * hs + 3) / 4); c->d_ss_d.shift = (ptrdiff_t) ((size_t) q_lo * hs); }
		else rc = c->d_ss_d.alloc_range(c, q_lo, q_hi + 1, m);
		if (rc) { c->d_ss_a.release(c); return rc; }      // (d_ss_a stands for both)
	}
	return FSEQ_OK;
}

void free_work(fseq_ctx *c)
{
	release_all(c, c->d_rank, c->d_keyd, c->d_nkeys, c->d_bstate_a, c->d_bstate_d, c->d_hrank, c->d_hkeyd, c->d_hnkeys, c->d_hstate_a, c->d_hstate_d);
	release_levels(c);
	release_all(c, c->d_ent, c->d_hdr, c->d_flags, c->d_recent, c->d_chunk_r0, c->d_tau, c->d_bk, c->d_bkws, c->d_todo, c->d_colmask, c->d_btws, c->d_only, c->d_tb);
	release_all(c, c->dp.M, c->dp.LB, c->dp.SZ, c->dp.K, c->dp.Tb, c->dp.Tbv, c->d_Mprev, c->d_spec);
	release_all(c, c->d_cols, c->d_grp, c->d_src, c->d_ss_a, c->d_ss_d, c->d_bs_w, c->d_bs_h, c->d_wgblk, c->d_wggrp, c->d_snap_a, c->d_snap_d, c->d_ws, c->d_cshist, c->d_cw_stats, c->d_p2keys, c->d_p2keys_flag);
	release_all(c, c->d_red_cnt, c->d_red_cnt_plan, c->d_red_vmin, c->d_red_rows, c->d_red_leaf, c->d_red_a, c->d_red_d, c->d_red_invalid, c->d_red_blocks, c->d_red_msa, c->d_cls, c->d_cls_have, c->d_red_src);
	release_all(c, c->d_red_ss_a, c->d_red_ss_d, c->d_red_cls, c->d_red_headd, c->d_red_ncls, c->d_red_taskblk, c->d_red_wgtasks, c->d_red_p2grp);
	// what was planned for the buffers that are gone
	c->lw.col_lo = c->lw.col_hi = 0;
	c->colmask_ready = false;
	c->ss_pack = 0; c->ss_ids = false;       // (the form of the stride states: decided again where they are allocated)
	c->red.memory.forget_verdicts();
	c->red_cap = 0; c->red_ld = 0;
	c->red_active = false;
	c->p2keys_live = false;
	c->cls_on = c->cls_every = c->cls_read = c->cls_staged = false; c->cls_ld = 0;
}

namespace {

// Device-side input path (row N2): rows go up as they are (one copy per row), the alphabet scan
// (consecutive_alphabet_as_builder, generate_context.cc:135-147: dense codes in ascending byte order,
// Appendix B A2) and the row-major -> column-major transpose run on the GPU.
int upload_rows_device_impl(fseq_ctx *c, uint8_t const *const *rows)
{
	fseq_params const &p = c->p;
	uint64_t const k_lo = held_lo(c), nloc = held_hi(c) - k_lo;      // sharded: this rank's columns only
	size_t const total = (size_t) p.m * nloc;
	DevTemp<uint8_t> d_raw(c);
	DevTemp<uint32_t> d_present(c);
	int rc;
	if ((rc = d_raw.alloc(total + 16)) || (rc = d_present.alloc(8))) return rc;
	// (one copy per row from the caller's pageable memory: the runtime stages them at ~32 GB/s.  Measured and dropped in round 4:
	// eight host threads filling pinned staging buffers of their own, each with its stream -- BASELINE C3's 2.5 GB in 77 - 86 ms
	// against 78, C2's 250 MB in 39 against 30: the host copies into the pinned buffers are no faster than the runtime's own
	// staging, and the buffers cost ~10 ms to pin)
	for (uint32_t r = 0; r < p.m && nloc; ++r)
	{
		hipError_t const e = hipMemcpyAsync(d_raw + (size_t) r * nloc, rows[r] + k_lo, nloc, hipMemcpyHostToDevice, c->stream);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "row upload", e);
	}
	(void) hipMemsetAsync(d_present, 0, 32, c->stream);
	if (total) hipLaunchKernelGGL(k_presence, dim3(1024), dim3(256), 0, c->stream, d_raw, total, d_present);
	uint32_t present[8];
	hipError_t e = hipMemcpyAsync(present, d_present, 32, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "alphabet scan", e);
	if (c->sh.on)
	{
		// the alphabet is that of the whole alignment: one presence word per byte value, max over the ranks
		uint32_t pw[256];
		for (int b = 0; b < 256; ++b) pw[b] = (present[b >> 5] >> (b & 31)) & 1u;
		e = hipMemcpy(c->sh.xbuf, pw, sizeof(pw), hipMemcpyHostToDevice);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "alphabet exchange", e);
		if ((rc = shard_exchange(c, 256, 1))) return rc;
		e = hipMemcpy(pw, c->sh.xbuf, sizeof(pw), hipMemcpyDeviceToHost);
		if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "alphabet exchange", e);
		memset(present, 0, sizeof(present));
		for (int b = 0; b < 256; ++b) if (pw[b]) present[b >> 5] |= 1u << (b & 31);
	}
	CodeTable tab;
	memset(&tab, 0, sizeof(tab));
	uint32_t sigma = 0;
	for (int b = 0; b < 256; ++b)
		if ((present[b >> 5] >> (b & 31)) & 1u) { tab.code_of[b] = (uint8_t) sigma; c->code_to_byte[sigma] = (uint8_t) b; ++sigma; }
	c->sigma = sigma;
	if ((rc = alloc_msa(c))) return rc;
	if (nloc)
	{
		dim3 const grid((uint32_t) ((nloc + 63) / 64), (uint32_t) ((p.m + 63) / 64));
		hipLaunchKernelGGL(k_encode_transpose, grid, dim3(256), 0, c->stream, d_raw, tab, p.m, nloc, c->d_msa_own, c->ld, c->bsh);
	}
	e = hipGetLastError();
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	if (e != hipSuccess) return fail(c, FSEQ_E_HIP, "encode + transpose", e);
	c->have_input = true;
	return FSEQ_OK;
}

} // namespace

// (sharded: the upload contains an exchange -- the alphabet of the whole alignment -- so a rank that fails here, before or
// behind it, says so in the exchange the others make next instead of leaving them in a collective)
int upload_rows_device(fseq_ctx *c, uint8_t const *const *rows)
{
	int const rc = upload_rows_device_impl(c, rows);
	shard_post_failure(c, rc);
	return rc;
}

int set_alphabet_and_upload(fseq_ctx *c, uint8_t const *base, size_t rs, size_t cs)
{
	fseq_params const &p = c->p;
	bool present[256] = {false};
	for (uint32_t r = 0; r < p.m; ++r)
	{
		uint8_t const *row = base + (size_t) r * rs;
		for (uint64_t col = 0; col < p.n; ++col) present[row[col * cs]] = true;
	}
	// consecutive_alphabet_as_builder: dense codes in ascending byte order (generate_context.cc:135-147, A2)
	uint8_t code_of[256] = {0};
	uint32_t sigma = 0;
	for (int b = 0; b < 256; ++b)
		if (present[b]) { code_of[b] = (uint8_t) sigma; c->code_to_byte[sigma] = (uint8_t) b; ++sigma; }
	c->sigma = sigma;
	int rc = alloc_msa(c);
	if (rc) return rc;
	// encode + transpose on the host in column tiles, then one copy per tile
	size_t const tile = std::max<size_t>(1, (size_t) (8u << 20) / c->ld);
	std::vector<uint8_t> buf(tile * c->ld);
	uint32_t const bsh = c->bsh, smask = (1u << bsh) - 1u, bits = 8u >> bsh;
	for (uint64_t c0 = held_lo(c); c0 < held_hi(c); c0 += tile)
	{
		uint64_t const c1 = std::min<uint64_t>(held_hi(c), c0 + tile);
		std::fill(buf.begin(), buf.end(), 0);
		for (uint32_t r = 0; r < p.m; ++r)
		{
			uint8_t const *row = base + (size_t) r * rs;
			for (uint64_t col = c0; col < c1; ++col)
				buf[(col - c0) * c->ld + (r >> bsh)] |= (uint8_t) (code_of[row[col * cs]] << ((r & smask) * bits));
		}
		HIP_TRY(c, hipMemcpy(c->d_msa + c0 * c->ld, buf.data(), (c1 - c0) * c->ld, hipMemcpyHostToDevice));
	}
	c->have_input = true;
	return FSEQ_OK;
}

// ---- sharded runs: the one exchange primitive (include/fseq.h, fseq_set_shard) -------------------------------
// all-reduce of xbuf[0 .. words) over the ranks through the caller's function; the data must already be queued
// into xbuf on c->stream.  Not sharded: nothing to do.
// Every exchange starts with a one-word maximum of the ranks' status words (the last word of the buffer): a rank that
// has failed (out of memory, a HIP error) posts its error code there ONCE, in the exchange the others make next, and
// every rank leaves with FSEQ_E_PEER instead of waiting in a collective for a rank that will never arrive.

namespace {

int shard_status(fseq_ctx *c, uint32_t mine)
{
	Shard &sh = c->sh;
	uint64_t const slot = sh.xwords - 1;
	HIP_TRY(c, hipMemcpyAsync(sh.xbuf + slot, &mine, 4, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (sh.fn(sh.user, slot, 1, 1) != 0) return fail(c, FSEQ_E_HIP, "the caller's all-reduce failed");
	uint32_t got = 0;
	HIP_TRY(c, hipMemcpy(&got, sh.xbuf + slot, 4, hipMemcpyDeviceToHost));
	if (got && !mine)
	{
		char what[96];
		snprintf(what, sizeof(what), "another rank of the sharded run failed (its error code: %u)", got);
		return fail(c, FSEQ_E_PEER, what);
	}
	return FSEQ_OK;
}

} // namespace

int shard_exchange(fseq_ctx *c, uint64_t words, int op)
{
	if (!c->sh.on) return FSEQ_OK;
	if (words + 1 > c->sh.xwords) return fail(c, FSEQ_E_ARG, "exchange buffer too small (fseq_shard_xbuf_words)");
	int rc = shard_status(c, 0);
	if (rc) return rc;
	HIP_TRY(c, hipStreamSynchronize(c->stream));
	if (c->sh.fn(c->sh.user, 0, words, op) != 0) return fail(c, FSEQ_E_HIP, "the caller's all-reduce failed");
	return FSEQ_OK;
}

// a rank that failed on its own tells the others (best effort: its device may be what failed)
void shard_post_failure(fseq_ctx *c, int code)
{
	if (!c->sh.on || code == FSEQ_OK || code == FSEQ_E_NO_REDUCTION || code == FSEQ_E_PEER) return;
	// once per context (the status exchange is a collective: a second post would have no partner), and not behind the
	// last exchange of a run (the other ranks have left)
	if (c->sh.posted || c->sh.closed) return;
	c->sh.posted = true;
	std::string const keep = c->err;
	(void) shard_status(c, (uint32_t) code);
	c->err = keep;
}

} // namespace fseq
