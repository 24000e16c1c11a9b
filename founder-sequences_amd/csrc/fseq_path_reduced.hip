// fseq_path_reduced.hip -- the segmentation path: [r5] phase C on representative rows (fseq_reduced.hpp) as the host sees it.
// The plan of one attempt -- the stages around plan_reduced (fseq_redplan.hpp) --, the launches of the reduced column kernel
// side by side, the redo marking, and the planner's host entry of include/fseq_debug.h.  Host code only: the unit
// instantiates no kernel and reaches every one through the launchers of csrc/fseq_reduced.hip (fseq_ctx.hpp).
#include "fseq_path.hpp"

namespace fseq {

namespace {

// bytes of each staged-column buffer of a reduced configuration: a column of the alignment (direct), of the reduced alignment at
// the rows the configuration holds, or -- cls_ld, [r10] -- the larger of that and a class column of phase A
uint32_t red_symcap(uint32_t m, uint32_t bsh, ReducedSet const &rs, bool direct, size_t cls_ld = 0)
{
	uint32_t const bytes = direct ? sym_bytes(m, bsh) : std::max<uint32_t>(sym_bytes(rs.rows, bsh), (uint32_t) cls_ld);
	return (bytes + 1023u) & ~1023u;                           // whole kilobytes: a wave stages sixteen bytes per lane
}

bool columns_fit_reduced(uint32_t m, uint32_t B, uint32_t bsh, ReducedSet const &rs, bool direct)
{
	// (value ids of a block -- its boundary values and one per column -- are 16-bit keys of the partition step)
	return rs.lds(B, red_symcap(m, bsh, rs, direct)) <= LDS_LIMIT && (uint64_t) rs.rows + B + 1u <= 65535u;
}

// the configurations as planning sees them, at this geometry
// cls_ld (a run that may stage phase A's class columns itself; needs the device): which of them take buffers of that width at no
// cost (red_cls_direct, fseq_redplan.hpp)
std::vector<RedConfig> red_configs(uint32_t m, uint32_t B, uint32_t bsh, bool direct, size_t cls_ld = 0)
{
	std::vector<RedConfig> out;
	for (int i = 0; i < reduced_config_count(); ++i)
	{
		ReducedSet rs;
		(void) reduced_config(i, &rs);
		RedConfig f{rs.rows, rs.values, rs.T, rs.E, rs.ew, columns_fit_reduced(m, B, bsh, rs, direct)};
		if (cls_ld && !direct && f.fits)
		{
			size_t const lds_rows = rs.lds(B, red_symcap(m, bsh, rs, false)), lds_cls = rs.lds(B, red_symcap(m, bsh, rs, false, cls_ld));
			if (lds_cls == lds_rows) f.cls = true;
			else if (lds_cls <= LDS_LIMIT && rs.prepare(lds_cls, !rs.phase_form()) == hipSuccess)
				f.cls = red_cls_direct(lds_cls, LDS_LIMIT, rs.resident(lds_rows), rs.resident(lds_cls));
		}
		out.push_back(f);
	}
	return out;
}

// [r10] this run's reduced column kernels may stage phase A's class columns themselves: phase A wrote some, in ids the 16-bit
// orders and the carried digit hold (at most 16,384 keys a block), and nobody asked for the gather
bool red_cls_stageable(fseq_ctx const *c)
{
	return c->cls_on && !c->red_direct && !c->tune.class_gather && ((uint64_t) c->cls_ld << c->bsh) <= 16384u;
}

// ... and no listed block reads the reduced alignment: every one has class columns and runs on configurations that take their width
bool red_needs_msa(fseq_ctx const *c)
{
	return !c->red_direct && !(red_cls_stageable(c) && c->cls_every && c->red.plan.gathered == 0u);
}

} // namespace

void red_fill_args(fseq_ctx *c, RedArgs &RA)
{
	RA.cnt = c->d_red_cnt; RA.vmin = c->d_red_vmin; RA.a = c->d_red_a; RA.d = c->d_red_d; RA.leaf = c->d_red_leaf;
	RA.invalid = c->d_red_invalid; RA.any_invalid = &red_flags(c)->unproven; RA.cap = c->red_cap; RA.m_true = c->p.m;
	RA.direct = c->red_direct ? 1u : 0u; RA.colbytes = sym_bytes(c->p.m, c->bsh); RA.rank = c->d_rank;
	RA.ss_a = c->d_red_ss_a; RA.ss_d = c->d_red_ss_d; RA.ss_stride = c->red_ss_stride; RA.ss_cap = c->red_ss_cap;
	RA.blocks = c->d_red_blocks;                               // (the plan's block lists: red_launch_all indexes them; pass 2 brings its own)
	// (the class columns, for the launches that stage them: red_launch_all sets cls_have where the configuration's buffers hold one)
	RA.cls_src = c->d_red_src; RA.nkeys = c->d_nkeys; RA.cls_msa = c->d_cls; RA.cls_ld = c->cls_ld;
}

namespace {

// ---- the stages of red_plan

// stage 1: the per-block buffers at this capacity.  A new capacity takes the remembered plan with it
int red_ensure_block_buffers(fseq_ctx *c, uint32_t cap)
{
	FSEQ_LONG_LOCALS(c);
	uint32_t const nbk = c->nblocks;
	if (c->d_red_cnt && c->red_cap == cap) return FSEQ_OK;
	// (the small per-block words for every block of the alignment; the per-block rows for my blocks only -- a rank of a
	// sharded run --, addressed by the block's place in the whole alignment like the key blocks and boundary states)
	if ((rc = c->d_red_cnt.alloc(c, nbk))) return rc;
	if ((rc = c->d_red_cnt_plan.alloc(c, nbk))) return rc;
	if ((rc = c->d_red_vmin.alloc(c, nbk))) return rc;
	if ((rc = c->d_red_invalid.alloc(c, nbk + 2))) return rc;
	if ((rc = c->d_red_blocks.alloc(c, 3 * (size_t) nbk))) return rc;
	if ((rc = c->d_red_src.alloc(c, nbk))) return rc;
	if ((rc = c->d_red_rows.alloc_range(c, b_lo, b_hi, cap))) return rc;
	if ((rc = c->d_red_leaf.alloc_range(c, b_lo, b_hi, cap))) return rc;
	if ((rc = c->d_red_a.alloc_range(c, b_lo, b_hi, cap))) return rc;
	if ((rc = c->d_red_d.alloc_range(c, b_lo, b_hi, cap))) return rc;
	c->red_cap = cap;
	c->red.memory.forget_plan();
	return FSEQ_OK;
}

// ... and what lives as long as the context: the pinned staging of a planning's two copies, the events of the side streams
int red_ensure_host(fseq_ctx *c)
{
	size_t const words = 6 * (size_t) c->nblocks + 64;      // (counts, the block lists, the class-column flags back, the blocks' sources out)
	if (c->red_pin_words < words)
	{
		if (c->h_red_pin) (void) hipHostFree(c->h_red_pin);
		c->h_red_pin = nullptr; c->red_pin_words = 0;
		HIP_TRY(c, hipHostMalloc(reinterpret_cast<void **>(&c->h_red_pin), words * 4, hipHostMallocDefault));
		c->red_pin_words = words;
	}
	if (!c->red_ev.fork)
		for (hipEvent_t *evt : c->red_ev.all()) HIP_TRY(c, hipEventCreateWithFlags(evt, hipEventDisableTiming));
	return FSEQ_OK;
}

// stage 2: k_reduce_prep leaves, per block of mine, the representatives and the reduced start state
int red_launch_prep(fseq_ctx *c, uint32_t X, uint32_t cap)
{
	FSEQ_LONG_LOCALS(c);
	// LDS-resident row counts: the representatives' symbols come from the alignment's own columns (a block stages whole columns)
	c->red_direct = !c->use_stream;
	RedPrepArgs A{};
	A.bstate_a = c->d_bstate_a; A.bstate_d = c->d_bstate_d; A.rank = c->d_rank; A.blocks = nullptr;
	A.m = m; A.B = c->B; A.L = (uint32_t) L; A.cap = cap; A.block0 = b_lo; A.leaf_only = 0; A.n = n; A.direct = c->red_direct ? 1u : 0u;
	A.Xp = X + (c->tune.reduced_margin >= 0 ? (uint32_t) c->tune.reduced_margin : X / 4u + 8u);
	A.cnt = c->d_red_cnt; A.vmin = c->d_red_vmin; A.rows = c->d_red_rows; A.leaf = c->d_red_leaf; A.a = c->d_red_a; A.d = c->d_red_d;
	A.invalid = c->d_red_invalid; A.flags = &red_flags(c)->unproven;      // (both words)
	HIP_TRY(c, launch_reduce_prep(st, my_blocks, A));
	return FSEQ_OK;
}

// the reduced alignment of the listed blocks (streamed rows), by the plan in force when it is queued
// The listed blocks are two lists by where their columns come from: the blocks with class columns (phase A's trie ranked them: d_cls_have) are
// gathered from those, the others (the trie gave them up) from the alignment as before.  Which block is which is known on the device when the
// launches are queued -- and a later run launches by its plan without waiting --, so both launches take the whole list and a workgroup
// of either leaves at once where the block is the other's; where the trie ran alone every block has class columns and the launch
// on the alignment is not made.
// [r10] Where the column kernels stage the class columns themselves (cls_staged), the gather from the class columns leaves out the blocks
// the plan sends there (d_red_src) and is not launched when there is none left; the reduced alignment is sized here, and only when a
// listed block reads it (a later run by the remembered plan may be the first that does: a block the trie gave up this time).
int red_reduce_msa(fseq_ctx *c)
{
	FSEQ_LONG_LOCALS(c);
	c->cls_staged = red_cls_stageable(c);
	if (!red_needs_msa(c)) { c->cls_read = true; return FSEQ_OK; }
	{
		// the reduced alignment (my columns only): column k at d_red_msa + k * red_ld
		uint32_t const max_rows = c->red.plan.max_rows;
		size_t const ldr = ((size_t) sym_bytes(max_rows ? max_rows : 1u, c->bsh) + 15) & ~size_t(15);
		uint64_t const k_lo = (uint64_t) b_lo * c->B, k_hi = std::min<uint64_t>(n, (uint64_t) b_hi * c->B);
		size_t const need = (size_t) (k_hi - k_lo) * ldr + 64;
		if (c->red_ld != ldr || c->d_red_msa.cap < need)
		{
			if ((rc = c->d_red_msa.ensure(c, need))) return rc;
			c->red_ld = ldr;
		}
		c->d_red_msa.rebase((ptrdiff_t) ((size_t) k_lo * c->red_ld));
	}
	ReducedMsaArgs D{c->d_red_msa, c->red_ld, c->d_red_cnt, c->d_red_rows, c->red_cap, c->d_red_blocks, c->red.plan.listed, c->red.plan.max_rows};
	if (c->cls_staged && c->red.plan.gathered == 0u) c->cls_read = true;      // (every block with class columns stages them: only the others are gathered)
	else
	{
		D.skip = c->cls_staged ? (uint32_t const *) c->d_red_src : nullptr;
		c->cls_read = c->cls_on && launch_reduce_cls(st, msa_args(c), D, ClassColumnArgs{c->d_cls, c->cls_ld, c->d_cls_have, c->d_red_leaf, c->d_rank});
		D.skip = nullptr;
		if (!c->cls_read) c->cls_staged = false;               // (a shape the gather does not take: phase A's columns are not read at all)
	}
	if (c->cls_read && c->cls_every) return FSEQ_OK;
	if (c->cls_read) { D.flag = c->d_cls_have; D.want = 0u; }
	launch_reduce_msa(st, msa_args(c), D, c->tune.reduced_msa_gather);
	return FSEQ_OK;
}

// stage 3: the remembered plan still holds: the device checks that the counts are the ones it was made from (the second of
// the RedFlags), and the reduced alignment is queued by it -- nothing waits
int red_queue_remembered(fseq_ctx *c)
{
	FSEQ_LONG_LOCALS(c);
	launch_reduce_check(st, c->d_red_cnt + b_lo, c->d_red_cnt_plan + b_lo, my_blocks, &red_flags(c)->unproven);      // (it sets the second word)
	if (!c->red_direct && (rc = red_reduce_msa(c))) return rc;
	c->tm.reduced_blocks = c->red.plan.reduced_blocks; c->tm.reduced_rows_mean = c->red.plan.rows_mean;
	return FSEQ_OK;
}

// stage 4: the counts come back (and stay on the device as what the plan was made from); with them, what planning is asked.
// From here on red.plan is being replaced: no remembered plan holds
int red_read_counts(fseq_ctx *c, RedPlanInput &in)
{
	FSEQ_LONG_LOCALS(c);
	uint32_t const nbk = c->nblocks;
	fseq_ctx::Red::Memory &M = c->red.memory;
	M.forget_plan();
	uint32_t *const h_cnt = c->h_red_pin;
	HIP_TRY(c, hipMemcpyAsync(h_cnt + b_lo, c->d_red_cnt + b_lo, (size_t) my_blocks * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipMemcpyAsync(c->d_red_cnt_plan + b_lo, c->d_red_cnt + b_lo, (size_t) my_blocks * 4, hipMemcpyDeviceToDevice, st));
	// [r10] (a planning waits for phase A anyway: which blocks the trie gave up is known here, not only in the run after -- where none
	// lacks class columns the reduced alignment may not be needed at all)
	uint32_t *const h_have = c->h_red_pin + 4 * (size_t) nbk;
	bool const ask_have = c->cls_on && !c->cls_every;
	if (ask_have) HIP_TRY(c, hipMemcpyAsync(h_have + b_lo, c->d_cls_have + b_lo, (size_t) my_blocks * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(c, hipStreamSynchronize(st));
	if (ask_have) c->cls_every = std::all_of(h_have + b_lo, h_have + b_hi, [](uint32_t h) { return h != 0u; });
	if (M.force.size() != nbk) M.force.assign(nbk, 0);
	in.m = m; in.nblocks = nbk; in.b_lo = b_lo; in.b_hi = b_hi;
	in.cnt.assign(nbk, RED_NONE);
	std::copy(h_cnt + b_lo, h_cnt + b_hi, in.cnt.begin() + b_lo);
	in.force = M.force;
	in.configs = red_configs(m, c->B, c->bsh, c->red_direct, red_cls_stageable(c) ? c->cls_ld : 0);
	in.reduced_always = c->tune.reduced_always;
	in.no_block_list = c->use_stream && !c->s2.T;
	return FSEQ_OK;
}

// [r10] the configuration's launches take staged-column buffers of the class width (the plan in force says so, and this run stages)
bool red_config_cls(fseq_ctx const *c, int config)
{
	return red_cls_stageable(c) && (size_t) config < c->red.cls_config.size() && c->red.cls_config[(size_t) config];
}

// FSEQ_DEBUG: what was planned
void red_report(fseq_ctx const *c, RedPlan const &P)
{
	uint32_t const m = c->p.m, my_blocks = P.reduced_blocks + P.nfull;
	fprintf(stderr, "[fseq] reduced phase C: %u of %u blocks on their representatives (mean %u of %u rows, most %u), %u on all rows\n", P.reduced_blocks, my_blocks,
	        P.rows_mean, m, P.max_rows, P.nfull);
	for (RedBin const &bin : P.bins)
	{
		uint64_t sr = 0;
		for (uint32_t i = 0; i < bin.count; ++i) sr += P.cnt[P.blocks[bin.first + i]];
		ReducedSet rs;
		(void) reduced_config(bin.config, &rs);
		bool const cls = red_config_cls(c, bin.config);
		size_t const lds = rs.lds(c->B, red_symcap(m, c->bsh, rs, c->red_direct, cls ? c->cls_ld : 0));
		uint32_t const res = rs.prepare(lds, !rs.phase_form()) == hipSuccess ? rs.resident(lds) : 0u;
		uint32_t staged = 0;
		for (uint32_t i = 0; i < bin.count; ++i) staged += P.from_cls[P.blocks[bin.first + i]];
		fprintf(stderr, "[fseq]   configuration of %u rows: %zu blocks, %llu representatives on average (%u threads x %u rows, %u distinct values, %zu bytes of LDS, %u workgroups per CU); columns: %s (%u of its blocks)\n",
		        rs.rows, (size_t) bin.count, (unsigned long long) (sr / bin.count), rs.T, rs.E, rs.values, lds, res,
		        c->red_direct ? "the alignment's own" : cls ? "phase A's class columns, staged by the kernel" : c->cls_on && c->tune.class_columns ? "the reduced alignment, gathered from the class columns" : "the reduced alignment, gathered from the alignment",
		        c->red_direct ? bin.count : cls ? staged : bin.count - staged);
	}
}

// stage 7: the reduced stride states, sized for the most representatives of a block
int red_size_buffers(fseq_ctx *c)
{
	FSEQ_LONG_LOCALS(c);
	uint32_t const max_rows = c->red.plan.max_rows;
	// (the reduced alignment: red_reduce_msa, where a listed block reads it)
	{
		// the reduced states for pass 2: every 8 columns (16: streamed rows), halfwords for the most representatives of a block
		// ([r16] two 16-bit arrays: the memory of the 32-bit states at twice these strides; FSEQ_RED_SS_STRIDE: a power of two, 4..64)
		uint32_t stride_ = c->use_stream ? 16u : 8u;
		if (c->tune.red_ss_stride) { stride_ = 4u; while (stride_ * 2u <= (uint32_t) std::min(c->tune.red_ss_stride, 64)) stride_ *= 2u; }
		uint32_t const scap = (std::max(max_rows, 1u) + 63u) & ~63u;
		uint64_t const q_lo = (uint64_t) b_lo * c->B / stride_, q_hi = std::min<uint64_t>(n, (uint64_t) b_hi * c->B) / stride_;
		size_t const halfwords = ((size_t) (q_hi - q_lo) + 2) * scap;
		if ((rc = c->d_red_ss_a.ensure(c, halfwords))) return rc;
		if ((rc = c->d_red_ss_d.ensure(c, halfwords))) return rc;
		c->red_ss_stride = stride_; c->red_ss_cap = scap;
		c->d_red_ss_a.rebase((ptrdiff_t) ((size_t) q_lo * scap));         // (the state at column q * stride at [q][scap])
		c->d_red_ss_d.rebase((ptrdiff_t) ((size_t) q_lo * scap));
	}
	return FSEQ_OK;
}

// stage 8: the plan's block lists to the device, through the pinned staging (behind the counts)
int red_upload_blocks(fseq_ctx *c)
{
	std::vector<uint32_t> const &blocks = c->red.plan.blocks;
	uint32_t *const h_blocks = c->h_red_pin + c->nblocks;
	std::copy(blocks.begin(), blocks.end(), h_blocks);
	HIP_TRY(c, hipMemcpyAsync(c->d_red_blocks, h_blocks, blocks.size() * 4, hipMemcpyHostToDevice, c->stream));
	// ... and every block's source
	uint32_t *const h_src = c->h_red_pin + 5 * (size_t) c->nblocks;
	std::copy(c->red.plan.from_cls.begin(), c->red.plan.from_cls.end(), h_src);
	HIP_TRY(c, hipMemcpyAsync(c->d_red_src, h_src, (size_t) c->nblocks * 4, hipMemcpyHostToDevice, c->stream));
	return FSEQ_OK;
}

} // namespace

// ---- [r5] phase C on representative rows (fseq_reduced.hpp): the plan of one attempt.
// k_reduce_prep leaves, per block, the representatives and the reduced start state.  The blocks are sorted into the
// configurations that hold them (a launch per configuration in use, side by side on their own streams) and the blocks
// that run on all rows: more representatives than any configuration holds (or than pay: > 70 % of the rows), or lists an
// earlier run on this input could not prove on the representatives (plan_reduced, fseq_redplan.hpp).  The first run on an input
// (or at a new capacity) reads the counts back and plans; later runs launch by the same plan without waiting and have the device
// check that the counts are the ones the plan was made from (flags word 1; the attempt is repeated with a fresh plan if not).
// *use: false when more than a quarter of the blocks would run on all rows anyway -- the attempt then takes the run on
// all rows with its stride states (diverse inputs).
int red_plan(fseq_ctx *c, uint32_t X, bool *use)
{
	FSEQ_LONG_LOCALS(c);
	fseq_ctx::Red::Memory &M = c->red.memory;
	*use = false;
	uint32_t cap = std::min<uint32_t>(m, 11264u);
	if (c->tune.reduced_cap) cap = std::min<uint32_t>(cap, (uint32_t) c->tune.reduced_cap);
	if ((rc = red_ensure_block_buffers(c, cap))) return rc;
	if (!my_blocks) return FSEQ_OK;                            // (a rank without blocks)
	// (the last run on this input at this capacity found the representatives not worth it: the same input gives the same answer)
	if (M.declined && M.declined_X == X && !c->tune.reduced_always) return FSEQ_OK;
	if ((rc = red_ensure_host(c))) return rc;
	if ((rc = red_launch_prep(c, X, cap))) return rc;
	if (M.plan_holds && M.plan_X == X && M.force.size() == c->nblocks)
	{
		if ((rc = red_queue_remembered(c))) return rc;
		*use = true;
		return FSEQ_OK;
	}
	RedPlanInput in;
	if ((rc = red_read_counts(c, in))) return rc;
	c->red.plan = plan_reduced(in);
	c->red.cls_config.assign(in.configs.size(), 0);
	for (size_t i = 0; i < in.configs.size(); ++i) c->red.cls_config[i] = in.configs[i].cls ? 1 : 0;
	RedPlan const &plan = c->red.plan;
	c->tm.reduced_blocks = plan.reduced_blocks; c->tm.reduced_rows_mean = plan.rows_mean;
	if (c->tune.debug) red_report(c, plan);
	switch (plan.verdict)
	{
	case RedVerdict::Declined:
		M.declined = true; M.declined_X = X;
		c->d_cls.release(c); c->cls_on = false;              // (phase A writes no class columns while the input stays declined)
		return FSEQ_OK;
	case RedVerdict::NoBlockList:
		// (nobody reads the class columns, and the same input gives the same answer next time: phase A writes none for it again)
		c->d_cls.release(c); c->cls_on = false; M.cls_unread = true;
		return FSEQ_OK;
	case RedVerdict::Use:
		break;
	}
	if ((rc = red_size_buffers(c))) return rc;
	if ((rc = red_upload_blocks(c))) return rc;
	if (!c->red_direct && (rc = red_reduce_msa(c))) return rc;
	M.plan_holds = true; M.plan_X = X;
	*use = true;
	return FSEQ_OK;
}

// launches of the reduced column kernel over lists of workgroups, one per configuration, side by side: the first on the
// context's stream, the others on streams of their own that wait for it and that it waits for

int red_launch_all(fseq_ctx *c, std::vector<RedLaunch> const &ls, RedArgs const &base, ListArgs const &lists)
{
	FSEQ_LONG_LOCALS(c);
	if (ls.empty()) return FSEQ_OK;
	// (up to RED_SIDE_STREAMS side streams, the context's second stream first -- every further hardware queue in use slows the
	// dependent launches of phase B, measured on BASELINE C3: 0.71 ms with none, 0.97 with three)
	size_t const nside = std::min<size_t>(ls.size() - 1, RED_SIDE_STREAMS);
	auto const joins = c->red_ev.joins();
	if (nside) HIP_TRY(c, hipEventRecord(c->red_ev.fork, st));
	// [r7] queued largest workgroups first (the blocks of ten thousand representatives are not the tail of the phase, as pass 2's
	// largest groups are not); the launch with the most blocks stays on the context's stream, the others take the side streams
	// in that order and, past those, the context's
	size_t main_i = 0;
	for (size_t i = 1; i < ls.size(); ++i) if (ls[i].count > ls[main_i].count) main_i = i;
	size_t side = 0;
	// the representatives' symbols: the alignment's own columns (LDS-resident row counts), or the reduced alignment
	ColumnsArgs C;
	C.A = msa_args(c);
	if (!c->red_direct) { C.A.msa = c->d_red_msa; C.A.ld = c->red_ld; }      // (not allocated where every block stages its class columns)
	C.lists = lists;
	for (size_t i = 0; i < ls.size(); ++i)
	{
		ReducedSet rs;
		(void) reduced_config(ls[i].config, &rs);
		RedArgs RA = base;
		// [r10] a configuration that takes the class width stages the class columns of its blocks that have them (and are planned so)
		bool const cls = c->cls_staged && red_config_cls(c, ls[i].config);
		RA.symcap = red_symcap(m, c->bsh, rs, c->red_direct, cls ? c->cls_ld : 0);
		RA.cls_have = cls ? (uint32_t const *) c->d_cls_have : nullptr;
		// [r16] pass 2's launches (the class tables asked for) take the sweep form
		bool const sweep = RA.cls != nullptr;
		size_t const lds = sweep ? rs.lds_sweep(c->B, RA.symcap) : rs.lds(c->B, RA.symcap);
		HIP_TRY(c, rs.prepare(lds, sweep));
		RA.blocks = base.blocks + ls[i].first;
		if (base.wg_tasks) RA.wg_tasks = base.wg_tasks + 3 * (size_t) ls[i].first;
		hipStream_t s_ = st;
		size_t const slot = (i != main_i && side < nside) ? side++ : nside;      // (nside: the context's stream)
		if (slot < nside)
		{
			if (slot >= 1 && !c->red_st[slot - 1]) HIP_TRY(c, hipStreamCreateWithFlags(&c->red_st[slot - 1], hipStreamNonBlocking));
			s_ = slot == 0 ? c->stream2 : c->red_st[slot - 1];
			HIP_TRY(c, hipStreamWaitEvent(s_, c->red_ev.fork, 0));
		}
		HIP_TRY(c, rs.launch(s_, ls[i].count, lds, C, RA));
		if (slot < nside) HIP_TRY(c, hipEventRecord(*joins[slot], s_));
	}
	for (size_t i = 0; i < nside; ++i) HIP_TRY(c, hipStreamWaitEvent(st, *joins[i], 0));
	HIP_TRY(c, hipGetLastError());
	return FSEQ_OK;
}

// the lists of the reduced blocks
int red_columns(fseq_ctx *c)
{
	RedArgs RA;
	red_fill_args(c, RA);
	std::vector<RedLaunch> ls;
	for (auto const &bin : c->red.plan.bins) ls.push_back(RedLaunch{bin.config, bin.first, bin.count});
	// (the bins ascend by the rows a workgroup holds: the largest first)
	std::reverse(ls.begin(), ls.end());
	return red_launch_all(c, ls, RA, list_args(c));
}

// the redo marking: the blocks of [b_lo, b_hi) whose lists the reduced phase C could not vouch for (d_red_invalid) run on all
// rows -- or, RED_WIDE, on the next configuration -- when the attempt runs again, and the plan goes with them.
// *count: the blocks marked; *wide: those of them that stay reduced
int red_take_invalid(fseq_ctx *c, uint32_t b_lo, uint32_t b_hi, uint32_t *count, uint32_t *wide)
{
	std::vector<uint32_t> inv(c->nblocks);
	HIP_TRY(c, hipMemcpy(inv.data(), c->d_red_invalid, (size_t) c->nblocks * 4, hipMemcpyDeviceToHost));
	*count = *wide = 0;
	for (uint32_t b = b_lo; b < b_hi; ++b)
		if (inv[b] && !c->red.plan.full[b]) { c->red.memory.force[b] = inv[b] == RED_WIDE ? RED_FORCE_WIDE : RED_FORCE_FULL; ++*count; *wide += inv[b] == RED_WIDE ? 1u : 0u; }
	if (*count) c->red.memory.forget_plan();
	return FSEQ_OK;
}

} // namespace fseq

using namespace fseq;

extern "C" {

int fseq_debug_red_plan(uint32_t m, uint32_t B, uint32_t bits, int direct, uint32_t nblocks, uint32_t b_lo, uint32_t b_hi, uint32_t const *cnt,
                        uint8_t const *force, int reduced_always, int no_block_list, uint32_t *configs, uint32_t *n_configs, int *verdict,
                        uint8_t *full, int32_t *config_of, int32_t *config_snap_of, uint32_t *blocks, uint32_t *n_blocks, uint32_t *bins,
                        uint32_t *n_bins, uint32_t *summary)
{
	if (!m || !B || (bits != 2 && bits != 4 && bits != 8) || (!cnt && nblocks) || b_lo > b_hi || b_hi > nblocks || nblocks > (1u << 24)) return FSEQ_E_ARG;
	for (uint32_t b = 0; b < nblocks; ++b)
		if ((cnt[b] > m && cnt[b] != RED_NONE) || (force && force[b] > RED_FORCE_WIDE)) return FSEQ_E_ARG;
	RedPlanInput in;
	in.m = m; in.nblocks = nblocks; in.b_lo = b_lo; in.b_hi = b_hi;
	in.cnt.assign(cnt, cnt + nblocks);
	if (force) in.force.assign(force, force + nblocks);
	else in.force.assign(nblocks, 0);
	in.configs = red_configs(m, B, bits == 2 ? 2u : bits == 4 ? 1u : 0u, direct != 0);
	in.reduced_always = reduced_always != 0;
	in.no_block_list = no_block_list != 0;
	if (in.configs.size() > FSEQ_DEBUG_RED_CONFIGS) return FSEQ_E_UNSUPPORTED;
	RedPlan const P = plan_reduced(in);
	if (n_configs) *n_configs = (uint32_t) in.configs.size();
	for (size_t i = 0; configs && i < in.configs.size(); ++i)
	{
		RedConfig const &f = in.configs[i];
		uint32_t const row[6] = {f.rows, f.values, f.T, f.E, f.ew ? 1u : 0u, f.fits ? 1u : 0u};
		std::copy(row, row + 6, configs + 6 * i);
	}
	if (verdict) *verdict = (int) P.verdict;
	if (full) std::copy(P.full.begin(), P.full.end(), full);
	if (config_of) std::copy(P.config_of.begin(), P.config_of.end(), config_of);
	if (config_snap_of) std::copy(P.config_snap_of.begin(), P.config_snap_of.end(), config_snap_of);
	if (blocks) std::copy(P.blocks.begin(), P.blocks.end(), blocks);
	if (n_blocks) *n_blocks = (uint32_t) P.blocks.size();
	for (size_t i = 0; bins && i < P.bins.size(); ++i)
	{
		bins[3 * i] = (uint32_t) P.bins[i].config; bins[3 * i + 1] = P.bins[i].first; bins[3 * i + 2] = P.bins[i].count;
	}
	if (n_bins) *n_bins = (uint32_t) P.bins.size();
	if (summary)
	{
		uint32_t const s[6] = {P.full_at, P.nfull, P.listed, P.max_rows, P.reduced_blocks, P.rows_mean};
		std::copy(s, s + 6, summary);
	}
	return FSEQ_OK;
}

int fseq_debug_red_cls_direct(uint32_t m, uint32_t B, uint32_t bits, uint64_t cls_ld, uint32_t config, uint32_t resident_rows, uint32_t resident_cls,
                              uint64_t *lds_rows, uint64_t *lds_cls, int *direct)
{
	if (!m || !B || (bits != 2 && bits != 4 && bits != 8) || !cls_ld || cls_ld > (1u << 20) || config >= (uint32_t) reduced_config_count()) return FSEQ_E_ARG;
	uint32_t const bsh = bits == 2 ? 2u : bits == 4 ? 1u : 0u;
	ReducedSet rs;
	(void) reduced_config((int) config, &rs);
	size_t const lr = rs.lds(B, red_symcap(m, bsh, rs, false)), lc = rs.lds(B, red_symcap(m, bsh, rs, false, (size_t) cls_ld));
	if (lds_rows) *lds_rows = lr;
	if (lds_cls) *lds_cls = lc;
	if (direct) *direct = (lc == lr || red_cls_direct(lc, LDS_LIMIT, resident_rows, resident_cls)) ? 1 : 0;
	return FSEQ_OK;
}

} // extern "C"
