// founder_sequences -- command line front end over the C ABI (include/fseq.h).
//
// Keeps the option surface, defaults and validation messages of the reference CLI
// (founder-sequences/cmdline.ggo:12-29, founder-sequences/main.cc:68-150) and the controller's
// input checks and outputs (founder-sequences/generate_context.cc:64-106,161-200,393-433).
// Host C++17 only; all segmentation work happens behind fseq_run_segmentation on the GPU.
// Joining: greedy (greedy_matcher.cc), bipartite-matching (bipartite_matcher.cc; an own Kuhn-Munkres
// in place of Lemon 1.3.1's MaxWeightedPerfectMatching) and random (join_context.cc:259-289).
#include <fseq.h>
#include "fseq_shard_rccl.hpp"

#include <fcntl.h>
#include <getopt.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <string>
#include <vector>

namespace {

enum class joining { BIPARTITE_MATCHING, GREEDY, RANDOM };
enum class input_format { FASTA, LIST_FILE };

char const *const USAGE =
	"Usage: founder_sequences --input=input-list.txt --segment-length-bound=... --output-founders=...\n"
	"Generate a segmentation in O(mn log sigma) time and output founder sequences.\n\n"
	"  -h, --help                         Print help and exit\n"
	"  -V, --version                      Print version and exit\n"
	"\nInput and output options:\n"
	"  -i, --input=PATH                   Input file path\n"
	"  -f, --input-format=FORMAT          Input file format  (possible values=\"FASTA\", \"list-file\" default=`list-file')\n"
	"  -e, --output-segments=PATH         Output segment co-ordinates in text format\n"
	"  -o, --output-founders=PATH         Founder file path\n"
	"      --output-matches=PATH          Match the input against the founders on the device and write the report of\n"
	"                                     match-sequences-to-founders (SEQUENCE_INDEX LB RB FOUNDER_INDICES; one GPU only)\n"
	"      --match-min-segment-length=N   ... closing a piece as soon as it has N columns  (default=`0': only where no founder continues)\n"
	"      --match-sequences=LIST         Match sequences that are not the input's -- a list file of sequences of the input's length, held\n"
	"                                     out of the segmentation -- against the founders on the device (one GPU only; not together\n"
	"                                     with --remove-identity-columns; requires --output-sequence-matches)\n"
	"      --output-sequence-matches=PATH ... and write the report of match-sequences-to-founders for them (honours\n"
	"                                     --match-min-segment-length; requires --match-sequences)\n"
	"      --hold-out=LIST                Hold sequences out of the segmentation: a comma list of 0-based indices in input order and of LO:HI ranges, both ends included (one GPU only)\n"
	"      --output-held-out-matches=PATH ... and match them against the founders on the device; the report's SEQUENCE_INDEX counts along LIST (requires --hold-out)\n"
	"      --remove-identity-columns      Segment only the columns in which the sequences differ and put the others back into the\n"
	"                                     founders from the first sequence (remove-identity-columns | founder_sequences |\n"
	"                                     insert-identity-columns in one run; segments in reduced co-ordinates; one GPU only)\n"
	"      --output-identity-columns=PATH ... and write the identity columns as a string of 0 / 1 (implies --remove-identity-columns)\n"
	"      --output-restored-matches=PATH ... and match the full-length input against the restored founders on the device: the report\n"
	"                                     of match-sequences-to-founders on the output of insert-identity-columns (requires\n"
	"                                     --remove-identity-columns; honours --match-min-segment-length)\n"
	"      --output-restored-segments=PATH ... and write the segments file in the input's co-ordinates on the device: LB / RB count the\n"
	"                                     input's columns and every substring has its identity columns back, from the first sequence\n"
	"                                     (requires --remove-identity-columns; every joining method; works under --upload-memory;\n"
	"                                     --output-segments, if given as well, stays in reduced co-ordinates)\n"
	"      --output-held-out-restored-matches=PATH  With --hold-out and --remove-identity-columns: match the full-length held-out\n"
	"                                     sequences against the restored founders on the device: the report of match-sequences-to-founders\n"
	"                                     for them and the founders file (SEQUENCE_INDEX counts along the --hold-out LIST; source\n"
	"                                     co-ordinates; honours --match-min-segment-length).  The two options combine only with this one\n"
	"      --output-sequence-restored-matches=PATH  With --match-sequences and --remove-identity-columns: the same for the sequences\n"
	"                                     of LIST, of the input's full length\n"
	"\nAlgorithm parameters:\n"
	"  -s, --segment-length-bound=SIZE    Segment length bound\n"
	"      --output-join-score=PATH       Score the join on the device and write, per border between two segments, how many founders\n"
	"                                     continue a substring that some sequence continues too, and per founder its breaks\n"
	"                                     (every joining method; works under --upload-memory, --hold-out and\n"
	"                                     --remove-identity-columns, there in reduced co-ordinates as --output-segments; one GPU only)\n"
	"      --output-graph=PATH            Write the founder block graph as GFA 1.0 from the device: an S line per distinct substring of every\n"
	"                                     segment, an L line per pair of substrings of adjacent segments that some sequence carries, with\n"
	"                                     the number of those sequences (needs the segmentation only: every joining method; works under\n"
	"                                     --upload-memory, --hold-out, --list-memory and --remove-identity-columns, there in reduced\n"
	"                                     co-ordinates as --output-segments; one GPU only)\n"
	"      --graph-paths                  ... with a P line per input sequence\n"
	"      --graph-gap-character=C        ... the character the S lines' substrings leave out; empty: every character stays  (default=`-')\n"
	"      --output-held-out-graph-threads=PATH  With --hold-out: thread the held-out sequences through the founder block graph on the\n"
	"                                     device and write, per sequence, the segments in which it carries a substring of the graph, the\n"
	"                                     borders it crosses along an edge and those it crosses as no input sequence does, and its walks\n"
	"                                     (needs the segmentation only: every joining method; works under --upload-memory and\n"
	"                                     --list-memory; one GPU only; not together with --remove-identity-columns)\n"
	"      --output-sequence-graph-threads=PATH  With --match-sequences: the same for the sequences of LIST\n"
	"      --output-held-out-graph-nearest=PATH  With --hold-out: for the held-out sequences, the nearest node of the founder block graph in\n"
	"                                     every segment and its distance in mismatched characters, on the device; per sequence the segments\n"
	"                                     admitted (at most --graph-nearest-max-distance mismatches) and exact, the borders crossed along an\n"
	"                                     edge and as no input sequence does, the walks and the mismatches (requirements and refusals of\n"
	"                                     --output-held-out-graph-threads; not for --remove-identity-columns or --gpus > 1)\n"
	"      --output-sequence-graph-nearest=PATH  With --match-sequences: the same for the sequences of LIST\n"
	"      --graph-nearest-max-distance=D ... the mismatches a segment may have and still be admitted to a walk  (default=`0')\n"
	"      --output-restored-graph=PATH   With --remove-identity-columns: the block graph in the input's co-ordinates -- the same L and P\n"
	"                                     lines, every S line's substring with its identity columns back, from the first sequence, and\n"
	"                                     lb / rb counting the input's columns (honours --graph-paths and --graph-gap-character; works\n"
	"                                     under --upload-memory and --reduce-on-upload; --output-graph, if given as well, stays in\n"
	"                                     reduced co-ordinates; one GPU only)\n"
	"      --output-held-out-restored-graph-threads=PATH  With --hold-out and --remove-identity-columns: thread the full-length held-out\n"
	"                                     sequences through that graph (the table of --output-held-out-graph-threads; columns count the\n"
	"                                     input's; one GPU only)\n"
	"      --output-sequence-restored-graph-threads=PATH  With --match-sequences and --remove-identity-columns: the same for the sequences\n"
	"                                     of LIST, of the input's full length (works under --reduce-on-upload)\n"
	"  -j, --segment-joining=METHOD       Segment joining method  (possible values=\"bipartite-matching\", \"greedy\", \"random\" default=`bipartite-matching')\n"
	"      --scan-segment-lengths=SPEC    Before anything else, write the maximum segment size at every segment length bound of SPEC --\n"
	"                                     a comma list of lengths, or LO:HI:STEP -- as a table (SEGMENT_LENGTH, MAX_SEGMENT_SIZE; one line\n"
	"                                     per distinct length, ascending) from the one resident alignment (one GPU only).  Alone: the\n"
	"                                     table and nothing else; with --segment-length-bound: the table, then the ordinary run\n"
	"      --output-scan=PATH             ... the table's path  (default: standard output)\n"
	"      --max-founders=K               ... and go on with the largest scanned bound whose maximum segment size is at most K (requires\n"
	"                                     --scan-segment-lengths; not together with --segment-length-bound)\n"
	"\nRunning options:\n"
	"  -m, --pbwt-sample-rate=q           On the first pass, store a PBWT sample every q*sqrt(n)-th position. Zero indicates no sampling.  (default=`4')\n"
	"      --random-seed=LONG             Seed for the random number generator  (default=`0')\n"
	"      --single-threaded              Use only one worker thread  (default=off)\n"
	"      --print-invocation             Print the command line arguments to stderr  (default=off)\n"
	"      --gpus=N                       Shard the alignment over the first N GPUs of this node (RCCL)  (default=`1')\n"
	"      --list-memory=MIB              Hold the per-column divergence lists in column windows of at most MIB MiB of device memory\n"
	"                                     (one GPU only; results are the same)  (default=`0': every list held)\n"
	"      --upload-memory=MIB            Read the sequence files of a list-file input in column chunks through at most MIB MiB of host\n"
	"                                     memory and as much device staging instead of loading them whole (list-file only; one GPU\n"
	"                                     only; results are the same; --output-segments then needs greedy joining)\n"
	"      --reduce-on-upload             With --upload-memory and --remove-identity-columns: find the columns in which all sequences agree\n"
	"                                     while the files are read and pack only the others, so that the device never holds the\n"
	"                                     full-length alignment (results are the same; not together with --hold-out)\n";

bool read_file(std::string const &path, std::string &out)
{
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
	return true;
}

// list-file: one path per line, each file holds one sequence (README.md:86)
bool read_list_file(char const *path, std::vector<std::string> &seqs)
{
	std::ifstream f(path);
	if (!f) { std::cerr << "Unable to open the input file '" << path << "'." << std::endl; return false; }
	std::string line;
	while (std::getline(f, line))
	{
		if (line.empty()) continue;
		std::string content;
		if (!read_file(line, content)) { std::cerr << "Unable to open the sequence file '" << line << "'." << std::endl; return false; }
		seqs.emplace_back(std::move(content));
	}
	return true;
}

// --upload-memory: the paths only; a file's length is its size (read_file takes a file's bytes as the sequence)
bool read_list_paths(char const *path, std::vector<std::string> &paths, std::vector<size_t> &lengths)
{
	std::ifstream f(path);
	if (!f) { std::cerr << "Unable to open the input file '" << path << "'." << std::endl; return false; }
	std::string line;
	while (std::getline(f, line))
	{
		if (line.empty()) continue;
		struct stat st;
		if (0 != stat(line.c_str(), &st) || !S_ISREG(st.st_mode)) { std::cerr << "Unable to open the sequence file '" << line << "'." << std::endl; return false; }
		paths.emplace_back(line);
		lengths.push_back((size_t) st.st_size);
	}
	return true;
}

// ... and the columns [c0, c0 + w) of every file into buf (row r at buf + r * w); one descriptor at a time
bool read_chunk(std::vector<std::string> const &paths, uint64_t c0, size_t w, uint8_t *buf, std::string &err)
{
	for (size_t r = 0; r < paths.size(); ++r)
	{
		int const fd(open(paths[r].c_str(), O_RDONLY));
		if (fd < 0) { err = "Unable to open the sequence file '" + paths[r] + "'."; return false; }
		size_t got(0);
		while (got < w)
		{
			ssize_t const k(pread(fd, buf + r * w + got, w - got, (off_t) (c0 + got)));
			if (k < 0 && EINTR == errno) continue;
			if (k <= 0) break;
			got += (size_t) k;
		}
		close(fd);
		if (got < w) { err = "Unable to read the sequence file '" + paths[r] + "' (it is shorter than when it was measured)."; return false; }
	}
	return true;
}

// the scan pass, then the encode pass, chunk after chunk through one host buffer of at most `bytes` and as much device staging
int upload_in_chunks(fseq_ctx *ctx, std::vector<std::string> const &paths, uint64_t n, uint64_t bytes, std::string &io_err)
{
	int rc(fseq_input_begin(ctx, nullptr, 0, bytes));
	if (FSEQ_OK != rc) return rc;
	size_t const m(paths.size());
	uint64_t width(fseq_input_chunk_columns(ctx));                // (two halves of bytes / 2: m x width is at most half the host's share)
	if ((width & ~63ull) >= 64) width &= ~63ull;
	if (width > n) width = n;
	std::vector<uint8_t> buf(m * (size_t) width);
	std::vector<uint8_t const *> at(m);
	for (int pass = 0; pass < 2; ++pass)
		for (uint64_t c0 = 0; c0 < n; c0 += width)
		{
			size_t const w((size_t) (n - c0 < width ? n - c0 : width));
			if (!read_chunk(paths, c0, w, buf.data(), io_err)) return FSEQ_E_ARG;
			for (size_t r = 0; r < m; ++r) at[r] = buf.data() + r * w;
			rc = pass ? fseq_input_columns(ctx, c0, w, at.data()) : fseq_input_scan(ctx, c0, w, at.data());
			if (FSEQ_OK != rc) return rc;
		}
	return fseq_input_end(ctx);
}

// --reduce-on-upload: the same two passes with the identity columns dropped on the way.  The scan pass finds them, the context over
// the other columns is made between the passes (*kept; it is src's until the end), and the second pass reads only the chunks that
// hold one of its columns
int upload_reduced_in_chunks(fseq_ctx *src, std::vector<std::string> const &paths, uint64_t n, uint64_t bytes, fseq_params const &pk, fseq_ctx **kept,
                             fseq_identity_summary *is, std::string &io_err)
{
	int rc(fseq_input_begin(src, nullptr, 0, bytes));
	if (FSEQ_OK != rc) return rc;
	size_t const m(paths.size());
	uint64_t width(fseq_input_chunk_columns(src));
	if ((width & ~63ull) >= 64) width &= ~63ull;
	if (width > n) width = n;
	std::vector<uint8_t> buf(m * (size_t) width);
	std::vector<uint8_t const *> at(m);
	for (int pass = 0; pass < 2; ++pass)
	{
		for (uint64_t c0 = 0; c0 < n; c0 += width)
		{
			size_t const w((size_t) (n - c0 < width ? n - c0 : width));
			uint64_t here(1);
			if (pass && FSEQ_OK != (rc = fseq_input_kept_columns(src, c0, w, &here))) return rc;
			if (!here) { if (FSEQ_OK != (rc = fseq_input_columns_kept(src, c0, w, nullptr))) return rc; continue; }
			if (!read_chunk(paths, c0, w, buf.data(), io_err)) return FSEQ_E_ARG;
			for (size_t r = 0; r < m; ++r) at[r] = buf.data() + r * w;
			rc = pass ? fseq_input_columns_kept(src, c0, w, at.data()) : fseq_input_scan_identity(src, c0, w, at.data());
			if (FSEQ_OK != rc) return rc;
		}
		if (!pass && FSEQ_OK != (rc = fseq_input_reduce(src, &pk, is))) return rc;
	}
	return fseq_input_end_kept(src, kept);
}

// FASTA: '>' header lines, sequence lines concatenated (README.md:80)
bool read_fasta(char const *path, std::vector<std::string> &seqs)
{
	std::ifstream f(path);
	if (!f) { std::cerr << "Unable to open the input file '" << path << "'." << std::endl; return false; }
	std::string line;
	bool open = false;
	while (std::getline(f, line))
	{
		if (!line.empty() && line.back() == '\r') line.pop_back();
		if (!line.empty() && line[0] == '>') { seqs.emplace_back(); open = true; continue; }
		if (!open) { if (line.empty()) continue; seqs.emplace_back(); open = true; }
		seqs.back() += line;
	}
	return true;
}

// --output-matches, --output-restored-matches: the report of the match the context holds, and a summary line
bool report_match(fseq_ctx *ctx, int rc, fseq_match_summary const &sm, char const *path)
{
	if (FSEQ_OK == rc) rc = fseq_write_match(ctx, path);
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return false; }
	std::cerr << "Matched the input against " << sm.n_founders << " founders: " << sm.pieces << " pieces, at most " << sm.max_pieces_per_row
	          << " in a sequence, " << sm.uncovered_cells << " uncovered cells." << std::endl;
	return true;
}

// --match-sequences: the held-out sequences against the founders the context has (permutations) or the rows given
// restored (--output-sequence-restored-matches): full-length sequences against the restored founders of the permutations
bool match_held_out(fseq_ctx *ctx, char const *list, size_t seq_length, uint32_t const *perm, uint8_t const *const *frows, uint32_t K,
                    unsigned long long min_len, char const *path, bool restored = false)
{
	std::cerr << "Matching the sequences of '" << list << "' against the founders…" << std::endl;
	std::vector<std::string> queries;
	if (!read_list_file(list, queries)) return false;
	if (queries.empty() || queries.size() > 0xFFFFFFFFull) { std::cerr << "No sequences to match in '" << list << "'." << std::endl; return false; }
	std::vector<uint8_t const *> qrows(queries.size());
	for (size_t i = 0; i < queries.size(); ++i)
	{
		if (queries[i].size() != seq_length) { std::cerr << "The sequences to match must have the length of the input's (" << seq_length << ")." << std::endl; return false; }
		qrows[i] = reinterpret_cast<uint8_t const *>(queries[i].data());
	}
	fseq_match_summary sm{};
	int const rc(restored ? fseq_match_rows_restored(ctx, perm, qrows.data(), (uint32_t) qrows.size(), min_len, &sm)
	                      : fseq_match_rows(ctx, perm, frows, K, qrows.data(), (uint32_t) qrows.size(), min_len, &sm));
	return report_match(ctx, rc, sm, path);
}

// --output-held-out-matches: the sequences --hold-out set aside, which the context holds on the device, against the founders the
// context has (permutations) or the rows given
bool match_context_held_out(fseq_ctx *ctx, uint32_t const *perm, uint8_t const *const *frows, uint32_t K, unsigned long long min_len, char const *path)
{
	std::cerr << "Matching the held-out sequences against the founders…" << std::endl;
	fseq_match_summary sm{};
	int const rc(fseq_match_held_out(ctx, perm, frows, K, min_len, &sm));
	return report_match(ctx, rc, sm, path);
}

std::ostream *open_out(char const *path, std::ofstream &file)
{
	if (!path || ('-' == path[0] && '\0' == path[1])) return &std::cout;
	file.open(path, std::ios::binary | std::ios::trunc);
	if (!file) { std::cerr << "Unable to open '" << path << "' for writing." << std::endl; std::exit(EXIT_FAILURE); }
	return &file;
}

// --scan-segment-lengths=SPEC: a comma list of positive lengths, or LO:HI:STEP (LO, LO + STEP, ... up to HI).  The distinct
// lengths, ascending; false where SPEC is malformed
bool parse_scan_spec(char const *spec, std::vector<uint64_t> &out)
{
	auto number = [](char const *&s, uint64_t &v) {
		if (!isdigit((unsigned char) *s)) return false;
		char *end = nullptr;
		errno = 0;
		v = strtoull(s, &end, 10);
		s = end;
		return errno != ERANGE && v > 0 && v < 0xFFFFFFF0ull;
	};
	char const *s = spec;
	out.clear();
	if (strchr(spec, ':'))
	{
		uint64_t lo = 0, hi = 0, step = 0;
		if (!number(s, lo) || *s++ != ':' || !number(s, hi) || *s++ != ':' || !number(s, step) || *s != '\0' || hi < lo) return false;
		if ((hi - lo) / step >= 1000000u) return false;
		for (uint64_t L = lo; L <= hi; L += step) out.push_back(L);
		return true;
	}
	while (true)
	{
		uint64_t v = 0;
		if (!number(s, v) || out.size() >= 1000000u) return false;
		out.push_back(v);
		if (*s == '\0') break;
		if (*s++ != ',') return false;
	}
	std::sort(out.begin(), out.end());
	out.erase(std::unique(out.begin(), out.end()), out.end());
	return true;
}

// --output-join-score: fseq_join_score on the permutations just made.  Tab-separated: a '#' line with the summary, one line per
// junction, a blank line, one line per founder.
bool write_join_score(fseq_ctx *ctx, fseq_result const &res, std::vector<uint32_t> const &perm, char const *path)
{
	size_t const pairs = res.segment_count ? (size_t) res.segment_count - 1 : 0;
	std::vector<fseq_join_score_entry> junctions(pairs);
	std::vector<uint32_t> breaks(res.max_segment_size);
	fseq_join_score_summary sm{};
	if (FSEQ_OK != fseq_join_score(ctx, perm.data(), junctions.data(), breaks.data(), nullptr, &sm)) { std::cerr << fseq_last_error(ctx) << std::endl; return false; }
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) { std::cerr << "Unable to open the join score output file." << std::endl; return false; }
	fprintf(f, "# JUNCTIONS=%llu\tSUPPORTED=%llu\tUNSUPPORTED=%llu\tGAPS=%llu\tROWS_THROUGH=%llu\tWEIGHT=%llu\tMIN_ROWS_THROUGH=%u\tMIN_ROWS_THROUGH_JUNCTION=%llu\tMAX_BREAKS=%u\n",
	        (unsigned long long) sm.junctions, (unsigned long long) sm.supported, (unsigned long long) sm.unsupported, (unsigned long long) sm.gaps,
	        (unsigned long long) sm.rows_through, (unsigned long long) sm.weight, sm.min_rows_through, (unsigned long long) sm.min_rows_through_junction, sm.max_breaks);
	fputs("JUNCTION\tRB\tSUPPORTED\tUNSUPPORTED\tGAPS\tROWS_THROUGH\tWEIGHT\n", f);
	for (size_t p = 0; p < pairs; ++p)
		fprintf(f, "%zu\t%llu\t%u\t%u\t%u\t%u\t%llu\n", p, (unsigned long long) junctions[p].rb, junctions[p].supported, junctions[p].unsupported, junctions[p].gaps,
		        junctions[p].rows_through, (unsigned long long) junctions[p].weight);
	fputs("\nFOUNDER\tBREAKS\n", f);
	for (size_t r = 0; r < breaks.size(); ++r) fprintf(f, "%zu\t%u\n", r, breaks[r]);
	bool ok = !ferror(f) && 0 == fflush(f);
	if (f != stdout && 0 != fclose(f)) ok = false;
	if (!ok) std::cerr << "Writing the join score output file failed." << std::endl;
	return ok;
}

// --output-held-out-graph-threads (list == nullptr: the sequences --hold-out set aside, which the context holds on the device) and
// --output-sequence-graph-threads (the sequences of `list`; n_held: the sequences held out): fseq_graph_thread_held_out / fseq_graph_thread_rows, statistics only.
// restored (--output-held-out-restored-graph-threads, --output-sequence-restored-graph-threads): the full-length sequences on a
// context over the columns in which the input's differ (fseq_graph_thread_held_out_restored / fseq_graph_thread_rows_restored).
// Tab-separated: a header, one line per sequence in the list's order, a last line '#' with the summary.
bool write_graph_threads(fseq_ctx *ctx, char const *list, size_t n_held, size_t seq_length, char const *path, bool restored = false)
{
	std::vector<std::string> queries;
	std::vector<uint8_t const *> qrows;
	size_t count = 0;
	if (list)
	{
		std::cerr << "Threading the sequences of '" << list << "' through the block graph…" << std::endl;
		if (!read_list_file(list, queries)) return false;
		if (queries.empty() || queries.size() > 0xFFFFFFFFull) { std::cerr << "No sequences to thread in '" << list << "'." << std::endl; return false; }
		qrows.resize(queries.size());
		for (size_t i = 0; i < queries.size(); ++i)
		{
			if (queries[i].size() != seq_length) { std::cerr << "The sequences to thread must have the length of the input's (" << seq_length << ")." << std::endl; return false; }
			qrows[i] = reinterpret_cast<uint8_t const *>(queries[i].data());
		}
		count = queries.size();
	}
	else
	{
		std::cerr << "Threading the held-out sequences through the block graph…" << std::endl;
		count = n_held;
	}
	std::vector<fseq_graph_thread_row> per_row(count);
	fseq_graph_thread_summary sm{};
	int const rc(restored ? (list ? fseq_graph_thread_rows_restored(ctx, qrows.data(), (uint32_t) count, nullptr, nullptr, per_row.data(), nullptr, &sm)
	                              : fseq_graph_thread_held_out_restored(ctx, nullptr, nullptr, per_row.data(), nullptr, &sm))
	             : list ? fseq_graph_thread_rows(ctx, qrows.data(), (uint32_t) count, nullptr, nullptr, per_row.data(), nullptr, &sm)
	                    : fseq_graph_thread_held_out(ctx, nullptr, nullptr, per_row.data(), nullptr, &sm));
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return false; }
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) { std::cerr << "Unable to open the graph threads output file." << std::endl; return false; }
	fputs("SEQUENCE_INDEX\tSEGMENTS\tMATCHED\tLINKED\tNOVEL\tWALKS\tLONGEST_WALK\tLONGEST_WALK_COLUMNS\tMATCHED_COLUMNS\n", f);
	for (size_t q = 0; q < count; ++q)
		fprintf(f, "%zu\t%llu\t%u\t%u\t%u\t%u\t%u\t%llu\t%llu\n", q, (unsigned long long) sm.segments, per_row[q].segments_matched, per_row[q].junctions_linked,
		        per_row[q].junctions_novel, per_row[q].walks, per_row[q].longest_walk_segments, (unsigned long long) per_row[q].longest_walk_columns,
		        (unsigned long long) per_row[q].columns_matched);
	fprintf(f, "#\tROWS=%llu\tSEGMENTS=%llu\tSEGMENTS_MATCHED=%llu\tJUNCTIONS_LINKED=%llu\tJUNCTIONS_NOVEL=%llu\tWALKS=%llu\tROWS_ON_GRAPH=%llu\n",
	        (unsigned long long) sm.rows, (unsigned long long) sm.segments, (unsigned long long) sm.segments_matched, (unsigned long long) sm.junctions_linked,
	        (unsigned long long) sm.junctions_novel, (unsigned long long) sm.walks, (unsigned long long) sm.rows_on_graph);
	bool ok = !ferror(f) && 0 == fflush(f);
	if (f != stdout && 0 != fclose(f)) ok = false;
	if (!ok) std::cerr << "Writing the graph threads output file failed." << std::endl;
	else std::cerr << "Threaded " << sm.rows << " sequences through the block graph: " << sm.rows_on_graph << " on the graph, " << sm.junctions_novel << " novel junctions." << std::endl;
	return ok;
}

// --output-held-out-graph-nearest (list == nullptr) and --output-sequence-graph-nearest: fseq_graph_nearest_held_out /
// fseq_graph_nearest_rows, statistics only.  Tab-separated: a header, one line per sequence, a last line '#' with the summary.
bool write_graph_nearest(fseq_ctx *ctx, char const *list, size_t n_held, size_t seq_length, uint32_t max_distance, char const *path)
{
	std::vector<std::string> queries;
	std::vector<uint8_t const *> qrows;
	size_t count = 0;
	if (list)
	{
		std::cerr << "Looking for the nearest nodes of the block graph for the sequences of '" << list << "'…" << std::endl;
		if (!read_list_file(list, queries)) return false;
		if (queries.empty() || queries.size() > 0xFFFFFFFFull) { std::cerr << "No sequences to thread in '" << list << "'." << std::endl; return false; }
		qrows.resize(queries.size());
		for (size_t i = 0; i < queries.size(); ++i)
		{
			if (queries[i].size() != seq_length) { std::cerr << "The sequences to thread must have the length of the input's (" << seq_length << ")." << std::endl; return false; }
			qrows[i] = reinterpret_cast<uint8_t const *>(queries[i].data());
		}
		count = queries.size();
	}
	else
	{
		std::cerr << "Looking for the nearest nodes of the block graph for the held-out sequences…" << std::endl;
		count = n_held;
	}
	std::vector<fseq_graph_nearest_row> per_row(count);
	fseq_graph_nearest_summary sm{};
	int const rc(list ? fseq_graph_nearest_rows(ctx, qrows.data(), (uint32_t) count, max_distance, nullptr, nullptr, nullptr, nullptr, per_row.data(), nullptr, &sm)
	                  : fseq_graph_nearest_held_out(ctx, max_distance, nullptr, nullptr, nullptr, nullptr, per_row.data(), nullptr, &sm));
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return false; }
	FILE *f = (path && strcmp(path, "-") != 0) ? fopen(path, "wb") : stdout;
	if (!f) { std::cerr << "Unable to open the graph nearest output file." << std::endl; return false; }
	fputs("SEQUENCE_INDEX\tSEGMENTS\tADMITTED\tEXACT\tLINKED\tNOVEL\tWALKS\tLONGEST_WALK\tLONGEST_WALK_COLUMNS\tADMITTED_COLUMNS\tMISMATCHES_ADMITTED\tMISMATCHES\tMAX_DISTANCE\n", f);
	for (size_t q = 0; q < count; ++q)
	{
		fseq_graph_nearest_row const &r = per_row[q];
		fprintf(f, "%zu\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%llu\t%llu\t%llu\t%llu\t%u\n", q, (unsigned long long) sm.segments, r.segments_admitted, r.segments_exact,
		        r.junctions_linked, r.junctions_novel, r.walks, r.longest_walk_segments, (unsigned long long) r.longest_walk_columns,
		        (unsigned long long) r.columns_admitted, (unsigned long long) r.mismatches_admitted, (unsigned long long) r.mismatches, r.max_distance);
	}
	fprintf(f, "#\tMAX_DISTANCE_ALLOWED=%u\tROWS=%llu\tSEGMENTS=%llu\tSEGMENTS_ADMITTED=%llu\tSEGMENTS_EXACT=%llu\tJUNCTIONS_LINKED=%llu\tJUNCTIONS_NOVEL=%llu\tWALKS=%llu\t"
	        "ROWS_ON_GRAPH=%llu\tMISMATCHES=%llu\n", max_distance, (unsigned long long) sm.rows, (unsigned long long) sm.segments, (unsigned long long) sm.segments_admitted,
	        (unsigned long long) sm.segments_exact, (unsigned long long) sm.junctions_linked, (unsigned long long) sm.junctions_novel, (unsigned long long) sm.walks,
	        (unsigned long long) sm.rows_on_graph, (unsigned long long) sm.mismatches);
	bool ok = !ferror(f) && 0 == fflush(f);
	if (f != stdout && 0 != fclose(f)) ok = false;
	if (!ok) std::cerr << "Writing the graph nearest output file failed." << std::endl;
	else std::cerr << "Nearest nodes of " << sm.rows << " sequences: " << sm.segments_exact << " of " << sm.rows * sm.segments << " segments exact, " << sm.mismatches << " mismatches, "
	               << sm.rows_on_graph << " sequences on the graph at " << max_distance << " mismatches a segment." << std::endl;
	return ok;
}

// --hold-out=LIST: a comma list of 0-based sequence indices and of LO:HI ranges, both ends included, in the order given.  false,
// with the reason in why, where LIST is malformed or names an index twice (whether the indices are below the sequence count is
// the caller's check, once the input is read)
bool parse_hold_out(char const *spec, std::vector<uint32_t> &out, std::string &why)
{
	auto number = [](char const *&s, uint64_t &v) {
		if (!isdigit((unsigned char) *s)) return false;
		char *end = nullptr;
		errno = 0;
		v = strtoull(s, &end, 10);
		s = end;
		return errno != ERANGE && v < 0xFFFFFFFFull;
	};
	char const *s = spec;
	out.clear();
	while (true)
	{
		uint64_t lo = 0, hi = 0;
		if (!number(s, lo)) { why = "malformed (a comma list of indices and LO:HI ranges is expected)"; return false; }
		hi = lo;
		if (*s == ':')
		{
			++s;
			if (!number(s, hi) || hi < lo) { why = "malformed (a range is LO:HI with LO <= HI)"; return false; }
		}
		if (hi - lo >= 0x7FFFFFFFull || out.size() + (hi - lo + 1) > 0x7FFFFFFFull) { why = "malformed (too many indices)"; return false; }
		for (uint64_t v = lo; v <= hi; ++v) out.push_back((uint32_t) v);
		if (*s == '\0') break;
		if (*s++ != ',') { why = "malformed (a comma list of indices and LO:HI ranges is expected)"; return false; }
	}
	std::vector<uint32_t> sorted(out);
	std::sort(sorted.begin(), sorted.end());
	if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { why = "names a sequence twice"; return false; }
	return true;
}

} // namespace

int main(int argc, char **argv)
{
	char const *hold_out_spec = nullptr, *out_held_matches = nullptr, *out_held_restored = nullptr, *out_seq_restored = nullptr;
	std::vector<uint32_t> held_rows;
	char const *input = nullptr, *out_segments = nullptr, *out_founders = nullptr, *out_matches = nullptr, *out_identity = nullptr, *out_restored_matches = nullptr, *out_restored_segments = nullptr;
	char const *match_seqs = nullptr, *out_seq_matches = nullptr, *out_join_score = nullptr;
	char const *out_graph = nullptr, *graph_gap = nullptr;
	char const *out_held_threads = nullptr, *out_seq_threads = nullptr;
	char const *out_held_nearest = nullptr, *out_seq_nearest = nullptr;
	unsigned long long nearest_max_distance = 0;
	bool nearest_max_distance_bad = false;
	char const *out_restored_graph = nullptr, *out_held_restored_threads = nullptr, *out_seq_restored_threads = nullptr;
	bool graph_paths = false;
	bool remove_identity = false;
	unsigned long long match_min_len = 0;
	bool match_min_len_bad = false;
	input_format fmt = input_format::LIST_FILE;
	joining join = joining::BIPARTITE_MATCHING;
	long seg_len = 0, sample_rate = 4, seed = 0;
	bool seg_len_given = false, single_threaded = false, print_invocation = false;
	long gpus = 1;
	bool gpus_given = false;
	unsigned long long list_memory_mib = 0;
	bool list_memory_bad = false;
	unsigned long long upload_mib = 0;
	bool upload_given = false, upload_bad = false, reduce_on_upload = false;
	char const *scan_spec = nullptr, *out_scan = nullptr;
	unsigned long long max_founders = 0;
	bool max_founders_given = false, max_founders_bad = false;

	static option const longopts[] = {
		{"help", no_argument, nullptr, 'h'}, {"version", no_argument, nullptr, 'V'},
		{"input", required_argument, nullptr, 'i'}, {"input-format", required_argument, nullptr, 'f'},
		{"output-segments", required_argument, nullptr, 'e'}, {"output-founders", required_argument, nullptr, 'o'},
		{"segment-length-bound", required_argument, nullptr, 's'}, {"segment-joining", required_argument, nullptr, 'j'},
		{"pbwt-sample-rate", required_argument, nullptr, 'm'}, {"random-seed", required_argument, nullptr, 1000},
		{"single-threaded", no_argument, nullptr, 1001}, {"print-invocation", no_argument, nullptr, 1002},
		{"gpus", required_argument, nullptr, 1003}, {"list-memory", required_argument, nullptr, 1004},
		{"output-matches", required_argument, nullptr, 1005}, {"match-min-segment-length", required_argument, nullptr, 1006},
		{"remove-identity-columns", no_argument, nullptr, 1007}, {"output-identity-columns", required_argument, nullptr, 1008},
		{"output-restored-matches", required_argument, nullptr, 1009}, {"upload-memory", required_argument, nullptr, 1010},
		{"scan-segment-lengths", required_argument, nullptr, 1011}, {"output-scan", required_argument, nullptr, 1012},
		{"max-founders", required_argument, nullptr, 1013},
		{"match-sequences", required_argument, nullptr, 1014}, {"output-sequence-matches", required_argument, nullptr, 1015},
		{"hold-out", required_argument, nullptr, 1016}, {"output-held-out-matches", required_argument, nullptr, 1017},
		{"output-held-out-restored-matches", required_argument, nullptr, 1018}, {"output-sequence-restored-matches", required_argument, nullptr, 1019},
		{"output-restored-segments", required_argument, nullptr, 1020}, {"reduce-on-upload", no_argument, nullptr, 1021},
		{"output-join-score", required_argument, nullptr, 1022},
		{"output-graph", required_argument, nullptr, 1023}, {"graph-paths", no_argument, nullptr, 1024},
		{"graph-gap-character", required_argument, nullptr, 1025},
		{"output-held-out-graph-threads", required_argument, nullptr, 1026}, {"output-sequence-graph-threads", required_argument, nullptr, 1027},
		{"output-held-out-graph-nearest", required_argument, nullptr, 1040}, {"output-sequence-graph-nearest", required_argument, nullptr, 1041},
		{"graph-nearest-max-distance", required_argument, nullptr, 1042},
		{"output-restored-graph", required_argument, nullptr, 1028},
		{"output-held-out-restored-graph-threads", required_argument, nullptr, 1029}, {"output-sequence-restored-graph-threads", required_argument, nullptr, 1030},
		{nullptr, 0, nullptr, 0}};
	int c;
	while ((c = getopt_long(argc, argv, "hVi:f:e:o:s:j:m:", longopts, nullptr)) != -1)
	{
		switch (c)
		{
			case 'h': std::cout << USAGE; return EXIT_SUCCESS;
			case 'V': std::cout << "founder_sequences (MI355X build, fseq ABI " << fseq_abi_version() << ")\n"; return EXIT_SUCCESS;
			case 'i': input = optarg; break;
			case 'f':
				if (0 == strcmp(optarg, "FASTA")) fmt = input_format::FASTA;
				else if (0 == strcmp(optarg, "list-file")) fmt = input_format::LIST_FILE;
				else { std::cerr << argv[0] << ": invalid argument, \"" << optarg << "\", for option `--input-format' (`-f')" << std::endl; return EXIT_FAILURE; }
				break;
			case 'e': out_segments = optarg; break;
			case 'o': out_founders = optarg; break;
			case 's': seg_len = strtol(optarg, nullptr, 10); seg_len_given = true; break;
			case 'j':
				if (0 == strcmp(optarg, "bipartite-matching")) join = joining::BIPARTITE_MATCHING;
				else if (0 == strcmp(optarg, "greedy")) join = joining::GREEDY;
				else if (0 == strcmp(optarg, "random")) join = joining::RANDOM;
				else { std::cerr << argv[0] << ": invalid argument, \"" << optarg << "\", for option `--segment-joining' (`-j')" << std::endl; return EXIT_FAILURE; }
				break;
			case 'm': sample_rate = strtol(optarg, nullptr, 10); break;
			case 1000: seed = strtol(optarg, nullptr, 10); break;
			case 1001: single_threaded = true; break;
			case 1002: print_invocation = true; break;
			case 1003: gpus = strtol(optarg, nullptr, 10); gpus_given = true; break;
			case 1004:
			{
				// a whole number of MiB, digits only (strtoull would take "-1" as a huge value)
				char *end = nullptr;
				errno = 0;
				list_memory_mib = strtoull(optarg, &end, 10);
				list_memory_bad = !isdigit((unsigned char) optarg[0]) || *end != '\0' || errno == ERANGE || list_memory_mib > (~0ull >> 20);
				break;
			}
			case 1005: out_matches = optarg; break;
			case 1006:
			{
				char *end = nullptr;
				errno = 0;
				match_min_len = strtoull(optarg, &end, 10);
				match_min_len_bad = !isdigit((unsigned char) optarg[0]) || *end != '\0' || errno == ERANGE;
				break;
			}
			case 1007: remove_identity = true; break;
			case 1008: out_identity = optarg; remove_identity = true; break;
			case 1009: out_restored_matches = optarg; break;
			case 1022: out_join_score = optarg; break;
			case 1023: out_graph = optarg; break;
			case 1024: graph_paths = true; break;
			case 1025: graph_gap = optarg; break;
			case 1026: out_held_threads = optarg; break;
			case 1027: out_seq_threads = optarg; break;
			case 1040: out_held_nearest = optarg; break;
			case 1041: out_seq_nearest = optarg; break;
			case 1042:
			{
				char *end = nullptr;
				errno = 0;
				nearest_max_distance = strtoull(optarg, &end, 10);
				nearest_max_distance_bad = !isdigit((unsigned char) optarg[0]) || *end != '\0' || errno == ERANGE || nearest_max_distance > 0xFFFFFFFFull;
				break;
			}
			case 1028: out_restored_graph = optarg; break;
			case 1029: out_held_restored_threads = optarg; break;
			case 1030: out_seq_restored_threads = optarg; break;
			case 1010:
			{
				// as --list-memory, but a positive number: 0 MiB hold no chunk
				char *end = nullptr;
				errno = 0;
				upload_mib = strtoull(optarg, &end, 10);
				upload_given = true;
				upload_bad = !isdigit((unsigned char) optarg[0]) || *end != '\0' || errno == ERANGE || 0 == upload_mib || upload_mib > (~0ull >> 20);
				break;
			}
			case 1011: scan_spec = optarg; break;
			case 1012: out_scan = optarg; break;
			case 1013:
			{
				char *end = nullptr;
				errno = 0;
				max_founders = strtoull(optarg, &end, 10);
				max_founders_given = true;
				max_founders_bad = !isdigit((unsigned char) optarg[0]) || *end != '\0' || errno == ERANGE || 0 == max_founders;
				break;
			}
			case 1014: match_seqs = optarg; break;
			case 1015: out_seq_matches = optarg; break;
			case 1016: hold_out_spec = optarg; break;
			case 1017: out_held_matches = optarg; break;
			case 1018: out_held_restored = optarg; break;
			case 1019: out_seq_restored = optarg; break;
			case 1020: out_restored_segments = optarg; break;
			case 1021: reduce_on_upload = true; break;
			default: return EXIT_FAILURE;
		}
	}
	if (!input) { std::cerr << argv[0] << ": '--input' ('-i') option required" << std::endl; return EXIT_FAILURE; }
	(void) single_threaded;

	// main.cc:80-115
	if (print_invocation)
	{
		std::cerr << "Invocation:";
		for (int i = 0; i < argc; ++i) std::cerr << ' ' << argv[i];
		std::cerr << std::endl;
	}
	if (seg_len_given)
	{
		if (seg_len <= 0) { std::cerr << "Segment length bound must be positive." << std::endl; return EXIT_FAILURE; }
	}
	else if (!scan_spec && !max_founders_given && !out_scan) { std::cerr << "Segment length bound needs to be specified when generating a segmentation." << std::endl; return EXIT_FAILURE; }
	std::vector<uint64_t> scan_lengths;
	if (scan_spec && !parse_scan_spec(scan_spec, scan_lengths))
	{ std::cerr << "The segment lengths to scan must be a comma list of positive numbers or LO:HI:STEP with LO <= HI and STEP positive." << std::endl; return EXIT_FAILURE; }
	if (out_scan && !scan_spec) { std::cerr << "--output-scan requires --scan-segment-lengths." << std::endl; return EXIT_FAILURE; }
	if (max_founders_bad) { std::cerr << "The maximum number of founders must be a positive number." << std::endl; return EXIT_FAILURE; }
	if (max_founders_given && !scan_spec) { std::cerr << "--max-founders requires --scan-segment-lengths (it chooses among the scanned segment length bounds)." << std::endl; return EXIT_FAILURE; }
	if (max_founders_given && seg_len_given) { std::cerr << "--max-founders is not supported together with --segment-length-bound (it chooses the bound itself)." << std::endl; return EXIT_FAILURE; }
	if (!(0 <= seed && (unsigned long) seed <= std::numeric_limits<std::uint_fast32_t>::max()))
	{ std::cerr << "Random seed out of bounds." << std::endl; return EXIT_FAILURE; }
	if (sample_rate <= 0) { std::cerr << "PBWT sample rate multiplier must be non-negative." << std::endl; return EXIT_FAILURE; }
	if (gpus < 1 || gpus > 64) { std::cerr << "The number of GPUs must be positive." << std::endl; return EXIT_FAILURE; }
	if (reduce_on_upload)
	{
		if (!upload_given) { std::cerr << "--reduce-on-upload requires --upload-memory (it drops the identity columns while the sequence files are read in chunks)." << std::endl; return EXIT_FAILURE; }
		if (!remove_identity) { std::cerr << "--reduce-on-upload requires --remove-identity-columns (it is another way to the same reduced run)." << std::endl; return EXIT_FAILURE; }
		if (hold_out_spec) { std::cerr << "--reduce-on-upload is not supported together with --hold-out (carrying the held-out sequences along needs the full-length alignment on the device)." << std::endl; return EXIT_FAILURE; }
		if (gpus > 1) { std::cerr << "--reduce-on-upload is not supported together with --gpus > 1 (the chunked input does not exchange the ranks' alphabets)." << std::endl; return EXIT_FAILURE; }
	}
	if (list_memory_bad) { std::cerr << "The list memory must be a non-negative number of MiB." << std::endl; return EXIT_FAILURE; }
	if (list_memory_mib && gpus > 1) { std::cerr << "--list-memory is not supported together with --gpus > 1." << std::endl; return EXIT_FAILURE; }
	if (match_min_len_bad) { std::cerr << "The minimum segment length of the match must be a non-negative number." << std::endl; return EXIT_FAILURE; }   // match-sequences-to-founders/main.cc:38-42
	if (out_matches && gpus > 1) { std::cerr << "--output-matches is not supported together with --gpus > 1 (a rank holds its own columns only)." << std::endl; return EXIT_FAILURE; }
	for (int k = 0; k < 2; ++k)
	{
		char const *const name = k ? "--output-sequence-graph-threads" : "--output-held-out-graph-threads";
		if (!(k ? out_seq_threads : out_held_threads)) continue;
		if (!(k ? match_seqs : hold_out_spec)) { std::cerr << name << " requires " << (k ? "--match-sequences." : "--hold-out.") << std::endl; return EXIT_FAILURE; }
		if (gpus > 1) { std::cerr << name << " is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only)." << std::endl; return EXIT_FAILURE; }
		if (remove_identity) { std::cerr << name << " is not supported together with --remove-identity-columns (the sequences would be threaded in reduced co-ordinates)." << std::endl; return EXIT_FAILURE; }
	}
	for (int k = 0; k < 2; ++k)
	{
		char const *const name = k ? "--output-sequence-restored-graph-threads" : "--output-held-out-restored-graph-threads";
		if (!(k ? out_seq_restored_threads : out_held_restored_threads)) continue;
		if (!((k ? match_seqs : hold_out_spec) && remove_identity)) { std::cerr << name << " requires " << (k ? "--match-sequences" : "--hold-out") << " and --remove-identity-columns." << std::endl; return EXIT_FAILURE; }
		if (gpus > 1) { std::cerr << name << " is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only)." << std::endl; return EXIT_FAILURE; }
	}
	if (nearest_max_distance_bad) { std::cerr << "--graph-nearest-max-distance must be a number from 0 to 4294967295." << std::endl; return EXIT_FAILURE; }
	for (int k = 0; k < 2; ++k)
	{
		char const *const name = k ? "--output-sequence-graph-nearest" : "--output-held-out-graph-nearest";
		if (!(k ? out_seq_nearest : out_held_nearest)) continue;
		if (!(k ? match_seqs : hold_out_spec)) { std::cerr << name << " requires " << (k ? "--match-sequences." : "--hold-out.") << std::endl; return EXIT_FAILURE; }
		if (gpus > 1) { std::cerr << name << " is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only)." << std::endl; return EXIT_FAILURE; }
		if (remove_identity) { std::cerr << name << " is not supported together with --remove-identity-columns (the sequences would be compared in reduced co-ordinates)." << std::endl; return EXIT_FAILURE; }
	}
	if (match_seqs && !out_seq_matches && !out_seq_restored && !out_seq_threads && !out_seq_restored_threads && !out_seq_nearest) { std::cerr << "--match-sequences requires --output-sequence-matches." << std::endl; return EXIT_FAILURE; }
	if (out_seq_matches && !match_seqs) { std::cerr << "--output-sequence-matches requires --match-sequences." << std::endl; return EXIT_FAILURE; }
	if (match_seqs && gpus > 1) { std::cerr << "--match-sequences is not supported together with --gpus > 1 (a rank holds its own columns only)." << std::endl; return EXIT_FAILURE; }
	if (out_seq_restored && !(match_seqs && remove_identity)) { std::cerr << "--output-sequence-restored-matches requires --match-sequences and --remove-identity-columns." << std::endl; return EXIT_FAILURE; }
	if (out_held_restored && !(hold_out_spec && remove_identity)) { std::cerr << "--output-held-out-restored-matches requires --hold-out and --remove-identity-columns." << std::endl; return EXIT_FAILURE; }
	// (the two combine with --remove-identity-columns only for the restored match; the reports in reduced co-ordinates stay refused)
	if (match_seqs && remove_identity && (!(out_seq_restored || out_seq_restored_threads) || out_seq_matches)) { std::cerr << "--match-sequences is not supported together with --remove-identity-columns (the match would be in reduced co-ordinates)." << std::endl; return EXIT_FAILURE; }
	if (out_join_score && gpus > 1) { std::cerr << "--output-join-score is not supported together with --gpus > 1 (a rank holds its own boundary states only)." << std::endl; return EXIT_FAILURE; }
	if (out_graph && gpus > 1) { std::cerr << "--output-graph is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only)." << std::endl; return EXIT_FAILURE; }
	if (out_restored_graph && gpus > 1) { std::cerr << "--output-restored-graph is not supported together with --gpus > 1 (a rank holds its own columns and boundary states only)." << std::endl; return EXIT_FAILURE; }
	if (out_restored_graph && !remove_identity) { std::cerr << "--output-restored-graph requires --remove-identity-columns (without it --output-graph is in the input's co-ordinates already)." << std::endl; return EXIT_FAILURE; }
	if ((graph_paths || graph_gap) && !out_graph && !out_restored_graph) { std::cerr << (graph_paths ? "--graph-paths" : "--graph-gap-character") << " requires --output-graph." << std::endl; return EXIT_FAILURE; }
	if (graph_gap && strlen(graph_gap) > 1) { std::cerr << "The gap character of the graph must be one character, or empty to keep every character." << std::endl; return EXIT_FAILURE; }
	if (out_restored_segments && gpus > 1) { std::cerr << "--output-restored-segments is not supported together with --gpus > 1 (a rank holds its own columns only)." << std::endl; return EXIT_FAILURE; }
	if (out_restored_segments && !remove_identity) { std::cerr << "--output-restored-segments requires --remove-identity-columns (without it --output-segments is in the input's co-ordinates already)." << std::endl; return EXIT_FAILURE; }
	if (remove_identity && gpus > 1) { std::cerr << "--remove-identity-columns is not supported together with --gpus > 1 (a rank holds its own columns only)." << std::endl; return EXIT_FAILURE; }
	if (out_restored_matches && !remove_identity) { std::cerr << "--output-restored-matches requires --remove-identity-columns (without it the founders are matched with --output-matches)." << std::endl; return EXIT_FAILURE; }
	if (remove_identity && out_matches) { std::cerr << "--remove-identity-columns is not supported together with --output-matches (the match would be in reduced co-ordinates)." << std::endl; return EXIT_FAILURE; }
	if (out_held_matches && !hold_out_spec) { std::cerr << "--output-held-out-matches requires --hold-out." << std::endl; return EXIT_FAILURE; }
	if (hold_out_spec)
	{
		std::string why;
		if (!parse_hold_out(hold_out_spec, held_rows, why)) { std::cerr << "The list of sequences to hold out is " << why << '.' << std::endl; return EXIT_FAILURE; }
		if (gpus > 1) { std::cerr << "--hold-out is not supported together with --gpus > 1 (a rank holds its own columns only)." << std::endl; return EXIT_FAILURE; }
		if (remove_identity && (!(out_held_restored || out_held_restored_threads) || out_held_matches)) { std::cerr << "--hold-out is not supported together with --remove-identity-columns (the held-out sequences would have to lose the same columns)." << std::endl; return EXIT_FAILURE; }
		if (scan_spec && !seg_len_given && !max_founders_given)
		{ std::cerr << "--hold-out with --scan-segment-lengths needs a segment length to go on with (--segment-length-bound or --max-founders): a scan alone writes its table and nothing else." << std::endl; return EXIT_FAILURE; }
	}

	if (upload_bad) { std::cerr << "The upload memory must be a positive number of MiB." << std::endl; return EXIT_FAILURE; }
	if (upload_given && input_format::FASTA == fmt) { std::cerr << "--upload-memory is not supported together with --input-format=FASTA (a FASTA file holds the sequences one after another, so a column chunk is not a range of its bytes; use list-file input)." << std::endl; return EXIT_FAILURE; }
	if (upload_given && gpus > 1) { std::cerr << "--upload-memory is not supported together with --gpus > 1 (the chunked input does not exchange the ranks' alphabets)." << std::endl; return EXIT_FAILURE; }
	if (upload_given && out_segments && joining::GREEDY != join) { std::cerr << "--upload-memory is not supported together with --output-segments under bipartite-matching or random joining (the segment texts need the raw rows on the host; greedy joining writes the header only)." << std::endl; return EXIT_FAILURE; }
	if (scan_spec && gpus > 1) { std::cerr << "--scan-segment-lengths is not supported together with --gpus > 1 (a sharded context's block geometry depends on the segment length)." << std::endl; return EXIT_FAILURE; }

	// generate_context.cc:64-106
	std::cerr << "Loading the input…" << std::flush;
	std::vector<std::string> seqs, paths;
	std::vector<size_t> lengths;
	if (upload_given)
	{
		// the files stay where they are: their sizes now, their bytes chunk by chunk when the context exists
		if (!read_list_paths(input, paths, lengths)) return EXIT_FAILURE;
	}
	else
	{
		if (!(input_format::FASTA == fmt ? read_fasta(input, seqs) : read_list_file(input, seqs))) return EXIT_FAILURE;
		for (auto const &s_ : seqs) lengths.push_back(s_.size());
	}
	if (lengths.empty()) { std::cerr << "\nThe input file contained no sequences." << std::endl; return EXIT_SUCCESS; }
	size_t const seq_length = lengths.front();
	std::cerr << " length: " << seq_length << std::endl;
	std::cerr << "Checking the input…" << std::endl;
	{
		bool stop = false;
		for (size_t i = 1; i < lengths.size(); ++i)
			if (lengths[i] != seq_length)
			{
				stop = true;
				std::cerr << "The length of the sequence at index " << i << " was " << lengths[i]
				          << " while that of the first one was " << seq_length << '.' << std::endl;
			}
		if (stop) return EXIT_FAILURE;
	}
	if (0 == seq_length) { std::cerr << "The sequences are empty." << std::endl; return EXIT_FAILURE; }
	if (hold_out_spec)
	{
		for (uint32_t r : held_rows)
			if (r >= lengths.size())
			{ std::cerr << "The list of sequences to hold out names index " << r << ", which is out of range: the input has " << lengths.size() << " sequences." << std::endl; return EXIT_FAILURE; }
		if (held_rows.size() >= lengths.size()) { std::cerr << "The list of sequences to hold out leaves no sequence to segment." << std::endl; return EXIT_FAILURE; }
	}

	fseq_params p{};
	p.m = (uint32_t) lengths.size();
	p.n = seq_length;
	// (a scan without a bound of its own: the context is made at the smallest scanned length; --max-founders sets the chosen one)
	p.segment_length = seg_len_given ? (uint64_t) seg_len : scan_lengths.front();
	bool const scan_only = scan_spec && !seg_len_given && !max_founders_given;
	p.pbwt_sample_rate = (uint64_t) sample_rate;
	std::vector<uint8_t const *> rows(lengths.size(), nullptr);      // (--upload-memory: no rows on the host)
	std::string io_err;
	for (size_t i = 0; i < seqs.size(); ++i) rows[i] = reinterpret_cast<uint8_t const *>(seqs[i].data());
	bool const sharded = gpus > 1 && p.n >= 2 * p.segment_length;      // (the short path is one sweep: it does not shard)
	if (gpus > 1 && !sharded) std::cerr << "The sequences are shorter than two segments; using one GPU." << std::endl;

	// One context per rank.  --gpus N: every rank on its own thread and device, RCCL for the exchanges
	// (fseq_shard_rccl.hpp); the ranks make the same calls in the same order and get the same result.
	fseq_host::rccl_world world;
	std::vector<fseq_ctx *> ctxs(sharded ? (size_t) gpus : 1, nullptr);
	std::vector<fseq_result> results(ctxs.size());
	int rc = FSEQ_OK;
	if (sharded || gpus_given)
	{
		// (--gpus 1 still makes the communicator and runs the one-word all-reduce: the transport is checked wherever it is asked for)
		std::string err;
		if (!world.init(sharded ? (int) gpus : 1, err) || !world.self_test(err)) { std::cerr << err << std::endl; return EXIT_FAILURE; }
		std::cerr << "RCCL: " << world.world() << " rank(s), self-test passed." << std::endl;
	}
	std::cerr << "Generating a compressed alphabet…" << std::endl;
	std::cerr << "Calculating the segmentation…" << std::endl;
	auto run_rank = [&](int r) -> int {
		fseq_params pr(p);
		pr.device = r;
		int rc_(fseq_create(&pr, &ctxs[r]));
		if (FSEQ_OK == rc_ && sharded) rc_ = world.attach(ctxs[r], r);
		if (sharded)
		{
			// Before the first collective the rank threads agree on the host: a rank without a context or an exchange buffer
			// (no device memory, ...) cannot take part in a status exchange, so everybody leaves here with its code.  From
			// here on a failing rank posts its code in the exchange the others make next (fseq.h: FSEQ_E_PEER).
			int const worst(world.agree(rc_));
			if (FSEQ_OK != worst) return FSEQ_OK != rc_ ? rc_ : FSEQ_E_PEER;
		}
		else if (FSEQ_OK != rc_) return rc_;
		if (list_memory_mib && FSEQ_OK != (rc_ = fseq_set_list_memory(ctxs[r], (uint64_t) list_memory_mib << 20))) return rc_;
		if (reduce_on_upload) {}                                   // (the input goes up where the identity columns are removed, below)
		else if (upload_given) { if (FSEQ_OK != (rc_ = upload_in_chunks(ctxs[r], paths, p.n, (uint64_t) upload_mib << 20, io_err))) return rc_; }
		else if (FSEQ_OK != (rc_ = fseq_set_rows(ctxs[r], rows.data()))) return rc_;     // (sharded: posts its own failures)
		if (hold_out_spec)
		{
			// the uploaded alignment is the source; the run goes on on a context over the other sequences, which keeps the held-out
			// ones aside on the device.  The source goes before the run: the two alignments and the lists need not fit the card together
			fseq_params pk(pr);
			pk.m = 0; pk.n = 0;
			fseq_ctx *sub(nullptr);
			fseq_hold_out_summary hs{};
			if (FSEQ_OK != (rc_ = fseq_create_without_rows(ctxs[r], held_rows.data(), (uint32_t) held_rows.size(), &pk, &sub, &hs))) return rc_;
			fseq_destroy(ctxs[r]);
			ctxs[r] = sub;
			std::cerr << "Held " << hs.held << " of " << hs.m_src << " sequences out of the segmentation." << std::endl;
			if (list_memory_mib && FSEQ_OK != (rc_ = fseq_set_list_memory(sub, (uint64_t) list_memory_mib << 20))) return rc_;
			// what the host holds of the sequences follows the kept ones' numbering from here on
			std::vector<uint32_t> kept(hs.kept);
			if (FSEQ_OK != (rc_ = fseq_get_held_out(sub, kept.data(), nullptr))) return rc_;
			for (size_t j = 0; j < kept.size(); ++j)               // (kept ascends: kept[j] >= j)
			{
				if (!seqs.empty() && kept[j] != j) seqs[j] = std::move(seqs[kept[j]]);
				if (!paths.empty() && kept[j] != j) paths[j] = std::move(paths[kept[j]]);
			}
			if (!seqs.empty()) seqs.resize(kept.size());
			if (!paths.empty()) paths.resize(kept.size());
			rows.assign(kept.size(), nullptr);
			for (size_t i = 0; i < seqs.size(); ++i) rows[i] = reinterpret_cast<uint8_t const *>(seqs[i].data());
			p.m = hs.kept;
		}
		if (remove_identity)
		{
			// the uploaded alignment is the source; the run goes on on a context over the columns in which the sequences differ
			fseq_params pk(pr);
			pk.m = 0; pk.n = 0;
			fseq_ctx *kept(nullptr);
			fseq_identity_summary is{};
			// (--hold-out: the held-out sequences go along, their kept columns and the identity columns in which they differ)
			// (--reduce-on-upload: the source context never holds an alignment; the kept columns are packed as the files are read)
			rc_ = reduce_on_upload ? upload_reduced_in_chunks(ctxs[r], paths, p.n, (uint64_t) upload_mib << 20, pk, &kept, &is, io_err)
			    : hold_out_spec ? fseq_create_without_identity_columns_held(ctxs[r], &pk, &kept, &is) : fseq_create_without_identity_columns(ctxs[r], &pk, &kept, &is);
			if (FSEQ_OK != rc_) return rc_;
			fseq_destroy(ctxs[r]);
			ctxs[r] = kept;
			std::cerr << "Removed " << is.identity << " of " << is.n << " columns in which all sequences agree." << std::endl;
			if (list_memory_mib && FSEQ_OK != (rc_ = fseq_set_list_memory(kept, (uint64_t) list_memory_mib << 20))) return rc_;
			if (out_identity && FSEQ_OK != (rc_ = fseq_write_identity_columns(kept, out_identity))) return rc_;
		}
		if (scan_spec)
		{
			// the table from the resident alignment (with --remove-identity-columns: the reduced one, lengths count kept columns)
			std::cerr << "Scanning " << scan_lengths.size() << " segment length bound(s)…" << std::endl;
			std::vector<fseq_length_scan_entry> entries(scan_lengths.size());
			for (size_t i = 0; i < entries.size(); ++i) entries[i].segment_length = scan_lengths[i];
			fseq_length_scan_summary ssm{};
			if (FSEQ_OK != (rc_ = fseq_scan_segment_lengths(ctxs[r], entries.data(), entries.size(), &ssm))) return rc_;
			std::ofstream scan_file;
			std::ostream &ts = *open_out(out_scan, scan_file);
			ts << "SEGMENT_LENGTH\tMAX_SEGMENT_SIZE\n";
			uint32_t smallest = ~0u;
			uint64_t chosen = 0;
			for (auto const &e : entries)                            // (ascending: parse_scan_spec)
			{
				ts << e.segment_length << '\t' << e.max_segment_size << '\n';
				smallest = std::min(smallest, e.max_segment_size);
				if (max_founders_given && e.max_segment_size <= max_founders) chosen = e.segment_length;
			}
			ts << std::flush;
			if (scan_only) return FSEQ_OK;
			if (max_founders_given)
			{
				if (!chosen)
				{
					io_err = "No scanned segment length bound gives at most " + std::to_string(max_founders) + " founders; the smallest maximum segment size seen was " + std::to_string(smallest) + ".";
					return FSEQ_OK;
				}
				std::cerr << "segment length bound chosen: " << chosen << std::endl;
				if (FSEQ_OK != (rc_ = fseq_set_segment_length(ctxs[r], chosen))) return rc_;
			}
		}
		return fseq_run_segmentation(ctxs[r], &results[r]);
	};
	if (sharded)
	{
		std::vector<int> const rcs(world.run(run_rank));
		for (size_t r = 0; r < rcs.size(); ++r)
			if (FSEQ_OK != rcs[r] && FSEQ_E_NO_REDUCTION != rcs[r])
			{
				// (a rank that failed on its own reports its error, the others FSEQ_E_PEER: print the cause)
				if (FSEQ_E_PEER != rcs[r] || FSEQ_OK == rc || FSEQ_E_PEER == rc) rc = rcs[r];
				std::cerr << "rank " << r << ": " << (ctxs[r] ? fseq_last_error(ctxs[r]) : fseq_strerror(rcs[r])) << std::endl;
			}
		if (FSEQ_OK == rc) rc = rcs[0];
		if (FSEQ_OK != rc && FSEQ_E_NO_REDUCTION != rc) return EXIT_FAILURE;
	}
	else
		rc = run_rank(0);
	fseq_ctx *ctx = ctxs[0];
	fseq_result res(results[0]);
	if (!ctx) { std::cerr << "Unable to initialise the GPU engine: " << fseq_strerror(rc) << std::endl; return EXIT_FAILURE; }
	if (FSEQ_E_NO_REDUCTION == rc)
	{
		// generate_context.cc:192-200
		std::cerr << "Unable to reduce the number of sequences; the maximum segment size is equal to the number of input sequences." << std::endl;
		return EXIT_FAILURE;
	}
	if (!io_err.empty()) { std::cerr << io_err << std::endl; return EXIT_FAILURE; }
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	if (scan_only)
	{
		std::cerr << "Done." << std::endl;
		fseq_destroy(ctx);
		return EXIT_SUCCESS;
	}

	std::ofstream founders_file, segments_file;
	if (res.short_path)
	{
		// generate_context.cc:161-176, segmentation_sp_context.cc:31-47
		std::vector<uint32_t> first(res.max_segment_size), len(res.max_segment_size);
		fseq_short_path_runs(ctx, first.data(), len.data());
		std::cerr << "Outputting…" << std::endl;
		std::ostream &os = *open_out(out_founders, founders_file);
		// (--upload-memory: the founders are input rows, read now from the files the runs name, one at a time)
		std::vector<std::string> named(upload_given && (out_matches || match_seqs || out_held_matches) ? res.max_segment_size : 0);
		for (uint32_t i = 0; i < res.max_segment_size; ++i)
		{
			std::string one;
			if (upload_given && (!read_file(paths[first[i]], one) || one.size() != seq_length))
			{ std::cerr << "Unable to read the sequence file '" << paths[first[i]] << "'." << std::endl; return EXIT_FAILURE; }
			os.write(upload_given ? one.data() : seqs[first[i]].data(), (std::streamsize) seq_length);
			os << '\n';
			if (!named.empty()) named[i] = std::move(one);
		}
		os << std::flush;
		if (out_segments)
		{
			std::ostream &ss = *open_out(out_segments, segments_file);
			ss << "SEQUENCE" "\n";
			for (uint32_t i = 0; i < res.max_segment_size; ++i) ss << len[i] << '\n';
			ss << std::flush;
		}
		if (out_matches)
		{
			// (no permutations on this path: the founders are the distinct rows just written)
			std::cerr << "Matching the input against the founders…" << std::endl;
			std::vector<uint8_t const *> frows(res.max_segment_size);
			for (uint32_t i = 0; i < res.max_segment_size; ++i) frows[i] = upload_given ? reinterpret_cast<uint8_t const *>(named[i].data()) : rows[first[i]];
			fseq_match_summary sm{};
			rc = fseq_match_founder_rows(ctx, frows.data(), res.max_segment_size, match_min_len, &sm);
			if (!report_match(ctx, rc, sm, out_matches)) return EXIT_FAILURE;
		}
		if (match_seqs && out_seq_matches)
		{
			std::vector<uint8_t const *> frows(res.max_segment_size);
			for (uint32_t i = 0; i < res.max_segment_size; ++i) frows[i] = upload_given ? reinterpret_cast<uint8_t const *>(named[i].data()) : rows[first[i]];
			if (!match_held_out(ctx, match_seqs, seq_length, nullptr, frows.data(), res.max_segment_size, match_min_len, out_seq_matches)) return EXIT_FAILURE;
		}
		if (out_held_restored || out_seq_restored)
		{
			std::cerr << "A match against the restored founders needs the permutations of a segmentation; the columns in which the sequences differ are fewer than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_restored_segments)
		{
			std::cerr << "--output-restored-segments needs the segments of a segmentation; the columns in which the sequences differ are fewer than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_join_score)
		{
			std::cerr << "--output-join-score needs the permutations of a segmentation; the sequences are shorter than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_graph)
		{
			std::cerr << "--output-graph needs the segments of a segmentation; the sequences are shorter than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_restored_graph)
		{
			std::cerr << "--output-restored-graph needs the segments of a segmentation; the columns in which the sequences differ are fewer than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_held_restored_threads || out_seq_restored_threads)
		{
			std::cerr << (out_held_restored_threads ? "--output-held-out-restored-graph-threads" : "--output-sequence-restored-graph-threads")
			          << " needs the segments of a segmentation; the columns in which the sequences differ are fewer than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_held_threads || out_seq_threads)
		{
			std::cerr << (out_held_threads ? "--output-held-out-graph-threads" : "--output-sequence-graph-threads") << " needs the segments of a segmentation; the sequences are shorter than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_held_nearest || out_seq_nearest)
		{
			std::cerr << (out_held_nearest ? "--output-held-out-graph-nearest" : "--output-sequence-graph-nearest") << " needs the segments of a segmentation; the sequences are shorter than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_restored_matches)
		{
			std::cerr << "--output-restored-matches needs the permutations of a segmentation; the columns in which the sequences differ are fewer than two segments." << std::endl;
			return EXIT_FAILURE;
		}
		if (out_held_matches)
		{
			// (last: the context holds one match at a time)
			std::vector<uint8_t const *> frows(res.max_segment_size);
			for (uint32_t i = 0; i < res.max_segment_size; ++i) frows[i] = upload_given ? reinterpret_cast<uint8_t const *>(named[i].data()) : rows[first[i]];
			if (!match_context_held_out(ctx, nullptr, frows.data(), res.max_segment_size, match_min_len, out_held_matches)) return EXIT_FAILURE;
		}
		std::cerr << "Done." << std::endl;
		fseq_destroy(ctx);
		return EXIT_SUCCESS;
	}

	// generate_context.cc:224-228
	std::cerr << "After calculating the traceback there were " << res.dp_segment_count
	          << " segments the maximum size of which was " << res.max_segment_size << '.' << std::endl;
	if (out_graph)
	{
		// the segmentation's own graph, from the context alone (no rows on the host, no join): in the co-ordinates --output-segments has
		std::cerr << "Outputting the block graph…" << std::endl;
		int const gap = graph_gap ? (graph_gap[0] ? (int) (unsigned char) graph_gap[0] : -1) : (int) '-';
		if (FSEQ_OK != (rc = fseq_write_block_graph(ctx, graph_paths ? FSEQ_GRAPH_PATHS : 0u, gap, out_graph))) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	}
	if (out_restored_graph)
	{
		// the same graph with its S lines in the input's co-ordinates, from what the device holds of the reduced context
		std::cerr << "Outputting the restored block graph…" << std::endl;
		int const gap = graph_gap ? (graph_gap[0] ? (int) (unsigned char) graph_gap[0] : -1) : (int) '-';
		if (FSEQ_OK != (rc = fseq_write_block_graph_restored(ctx, graph_paths ? FSEQ_GRAPH_PATHS : 0u, gap, out_restored_graph))) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	}
	// sequences that took no part in the segmentation through its graph, from the context alone (no join)
	if (out_held_threads && !write_graph_threads(ctx, nullptr, held_rows.size(), seq_length, out_held_threads)) return EXIT_FAILURE;
	if (out_seq_threads && !write_graph_threads(ctx, match_seqs, 0, seq_length, out_seq_threads)) return EXIT_FAILURE;
	if (out_held_nearest && !write_graph_nearest(ctx, nullptr, held_rows.size(), seq_length, (uint32_t) nearest_max_distance, out_held_nearest)) return EXIT_FAILURE;
	if (out_seq_nearest && !write_graph_nearest(ctx, match_seqs, 0, seq_length, (uint32_t) nearest_max_distance, out_seq_nearest)) return EXIT_FAILURE;
	// ... the full-length ones on a context over the columns in which the input's differ (seq_length is the input's)
	if (out_held_restored_threads && !write_graph_threads(ctx, nullptr, held_rows.size(), seq_length, out_held_restored_threads, true)) return EXIT_FAILURE;
	if (out_seq_restored_threads && !write_graph_threads(ctx, match_seqs, 0, seq_length, out_seq_restored_threads, true)) return EXIT_FAILURE;
	std::cerr << "Joining the remaining segments…" << std::endl;
	std::vector<uint32_t> perm((size_t) res.segment_count * res.max_segment_size);
	std::vector<uint32_t> all_a, all_d;                         // sharded: the boundary states, collected from their owners
	std::vector<fseq_segment> segments;
	if (sharded)
	{
		size_t const S(res.segment_count), m(p.m);
		segments.resize(S);
		if (FSEQ_OK != (rc = fseq_get_segments(ctx, segments.data()))) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
		all_a.resize(S * m); all_d.resize(S * m);
		std::vector<uint64_t> lbs(S), rbs(S);
		for (size_t i = 0; i < S; ++i)
		{
			lbs[i] = segments[i].lb; rbs[i] = segments[i].rb;
			uint32_t owner(0);
			if (FSEQ_OK != (rc = fseq_shard_owner(ctx, segments[i].rb, &owner)) ||
			    FSEQ_OK != (rc = fseq_boundary_state(ctxs[owner], i, all_a.data() + i * m, all_d.data() + i * m)))
			{ std::cerr << fseq_last_error(ctxs[owner < ctxs.size() ? owner : 0]) << std::endl; return EXIT_FAILURE; }
		}
		switch (join)
		{
			case joining::GREEDY: rc = fseq_greedy_match_host(p.m, res.max_segment_size, S, lbs.data(), rbs.data(), all_a.data(), all_d.data(), perm.data()); break;
			case joining::BIPARTITE_MATCHING: rc = fseq_bipartite_match_host(p.m, res.max_segment_size, S, lbs.data(), rbs.data(), all_a.data(), all_d.data(), perm.data(), nullptr); break;
			case joining::RANDOM: rc = fseq_random_join_host(p.m, res.max_segment_size, S, lbs.data(), rbs.data(), all_a.data(), all_d.data(), (uint32_t) seed, perm.data()); break;
		}
	}
	else
	switch (join)                                               // join_context.cc:130-160
	{
		case joining::GREEDY: rc = fseq_join_greedy(ctx, perm.data()); break;
		case joining::BIPARTITE_MATCHING: rc = fseq_join_bipartite(ctx, perm.data()); break;
		case joining::RANDOM: rc = fseq_join_random(ctx, (uint32_t) seed, perm.data()); break;
	}
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	std::cerr << "Outputting the founders…" << std::endl;
	// (not sharded: the lines are put together where the alignment already is, on the device; sharded: a rank holds its own columns)
	rc = sharded ? fseq_write_founders(ctx, rows.data(), perm.data(), out_founders)
	   : remove_identity ? fseq_write_founders_restored(ctx, perm.data(), out_founders) : fseq_write_founders_device(ctx, perm.data(), out_founders);
	if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	if (out_segments)
	{
		// segmentation_dp_arg.cc:13-104; with greedy joining the copy-number matrix is empty, so only the
		// header is written (join_context.cc:57-61, greedy_matcher.cc:468-476)
		std::cerr << "Outputting the segments…" << std::endl;
		int const how = joining::GREEDY == join ? FSEQ_JOIN_GREEDY : (joining::RANDOM == join ? FSEQ_JOIN_RANDOM : FSEQ_JOIN_BIPARTITE);
		// (not sharded: the lines are put together where the alignment and the boundary states already are, on the device --
		// no rows on the host needed, so --remove-identity-columns has its reduced rows without squeezing them here; what the
		// device writer does not serve goes to the host writer while the rows are on the host; under --upload-memory, which
		// reaches this point with greedy joining only, there are none)
		bool from_device = false;
		if (!sharded)
		{
			rc = fseq_write_segments_device(ctx, how, out_segments);
			from_device = FSEQ_OK == rc;
			if (!from_device && !(FSEQ_E_UNSUPPORTED == rc && !upload_given)) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
		}
		if (!from_device && remove_identity)
		{
			// the segments are in reduced co-ordinates: the rows without their identity columns, as the chain of tools has them
			std::vector<uint8_t> mask(seq_length);
			if (FSEQ_OK != (rc = fseq_get_identity_columns(ctx, mask.data(), nullptr))) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
			for (auto &s_ : seqs)
			{
				size_t k(0);
				for (size_t i = 0; i < seq_length; ++i) if (!mask[i]) s_[k++] = s_[i];
				s_.resize(k);
			}
			for (size_t i = 0; i < seqs.size(); ++i) rows[i] = reinterpret_cast<uint8_t const *>(seqs[i].data());
		}
		if (!from_device)
			rc = sharded ? fseq_write_segments_host(ctx, rows.data(), how, all_a.data(), all_d.data(), out_segments)
			             : fseq_write_segments(ctx, rows.data(), how, out_segments);
		if (FSEQ_OK != rc) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	}
	if (out_join_score)
	{
		// what the join is worth, from the context alone (no rows on the host): in the co-ordinates --output-segments has
		std::cerr << "Scoring the join…" << std::endl;
		if (!write_join_score(ctx, res, perm, out_join_score)) return EXIT_FAILURE;
	}
	if (out_restored_segments)
	{
		// the same file in the input's co-ordinates, from what the device holds of the reduced context: no rows on the host, so
		// every joining method is served under --upload-memory too
		std::cerr << "Outputting the restored segments…" << std::endl;
		int const how = joining::GREEDY == join ? FSEQ_JOIN_GREEDY : (joining::RANDOM == join ? FSEQ_JOIN_RANDOM : FSEQ_JOIN_BIPARTITE);
		if (FSEQ_OK != (rc = fseq_write_segments_restored(ctx, how, out_restored_segments))) { std::cerr << fseq_last_error(ctx) << std::endl; return EXIT_FAILURE; }
	}
	if (out_matches)
	{
		std::cerr << "Matching the input against the founders…" << std::endl;
		fseq_match_summary sm{};
		rc = fseq_match_founders(ctx, perm.data(), match_min_len, &sm);
		if (!report_match(ctx, rc, sm, out_matches)) return EXIT_FAILURE;
	}
	if (match_seqs && out_seq_matches && !match_held_out(ctx, match_seqs, seq_length, perm.data(), nullptr, 0, match_min_len, out_seq_matches)) return EXIT_FAILURE;
	if (out_seq_restored && !match_held_out(ctx, match_seqs, seq_length, perm.data(), nullptr, 0, match_min_len, out_seq_restored, true)) return EXIT_FAILURE;
	if (out_restored_matches)
	{
		// the last step of the chain: the full-length input against the founders just written, in the source's co-ordinates
		std::cerr << "Matching the input against the restored founders…" << std::endl;
		fseq_match_summary sm{};
		rc = fseq_match_founders_restored(ctx, perm.data(), match_min_len, &sm);
		if (!report_match(ctx, rc, sm, out_restored_matches)) return EXIT_FAILURE;
	}
	if (out_held_matches && !match_context_held_out(ctx, perm.data(), nullptr, 0, match_min_len, out_held_matches)) return EXIT_FAILURE;      // (last: one match at a time)
	if (out_held_restored)
	{
		std::cerr << "Matching the held-out sequences against the restored founders…" << std::endl;
		fseq_match_summary sm{};
		rc = fseq_match_held_out_restored(ctx, perm.data(), match_min_len, &sm);
		if (!report_match(ctx, rc, sm, out_held_restored)) return EXIT_FAILURE;
	}
	std::cerr << "Done." << std::endl;
	for (fseq_ctx *c_ : ctxs) if (c_) fseq_destroy(c_);
	return EXIT_SUCCESS;
}
