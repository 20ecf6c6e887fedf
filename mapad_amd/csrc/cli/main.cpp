// mapad-amd — command line with the `mapad index` / `mapad map` flag surface (src/main.rs:57-302) on top of the C ABI
// (include/mapad_amd.h).  Everything a Rust `mapad` would do around the hot path is done here through the same extern "C"
// calls a Rust caller would bind: index open/build, parameters, mapad_map_batch (GPU), mapad_hits_to_records_gpu (SA locate on the GPU), BAM output.
//
//   mapad-amd [--seed N] [--devices K] index -g ref.fa
//   mapad-amd [--devices K] worker --host H [--port 3130] [--dry_run]
//   mapad-amd [--seed N] [--devices 0-7 | 0,1,...] map -r reads.{bam,cram,fastq,fastq.gz} -g ref.fa -o out.bam -l single_stranded|double_stranded
//             -p 0.03 | (-c CUTOFF [-e EXP]) -f F -t T -d D -s S [-D 0.02] -i I [-x 1.0] [--batch_size 250000] [--coalesce 1 (4 on a text of >= 2^31 rows)] [--coalesce_steady N (= --coalesce)] [--in_flight 4] [--ignore_base_quality]
//             [--collapse_duplicates (map each distinct read of a chunk once; same output)]
//             [--damage_profile FILE [--damage_profile_unique] (substitution counts by distance from the reads' ends, counted on the GPU; same BAM)]
//             [--coverage FILE [--coverage_unique] (per-contig breadth and depth and the depth histogram of the reported alignments, counted on the GPU; same BAM)]
//             [--mark_duplicates | --exclude_duplicates] [--duplicates FILE] (PCR duplicates by start, span and strand of the reported alignment get 0x400 in the BAM, the first
//              read in input order being the original; --exclude_duplicates also leaves them out of the three tables below; FILE: the counts and the histogram of copies per
//              fragment.  One device only)
//             [--damage_score [--damage_score_min X] [--damage_score_hist FILE]] (per-read damage score: the log-likelihood ratio, in bits, of the reported alignment under the damage
//              model -f/-t/-d/-s against the same model without damage, computed on the GPU; every mapped record gets DS:f.  --damage_score_min X also leaves the reads scoring
//              below X out of the three tables below; FILE: the summary and the 128 half-bit bins.  With --devices every device scores its own reads)
//             [--rescale_qualities [--rescale_pileup] [--rescale_keep_original] [--rescale_report FILE]] (base qualities marked down at likely-damaged bases on the GPU: QUAL of a
//              C->T / G->A mismatch of a mapped record drops by the posterior, under the damage model -f/-t/-d/-s, that the mismatch is damage — mapDamage's rescaling rule.
//              --rescale_pileup also lets --pileup_min_bq see the rescaled qualities (needs --pileup or --consensus); --rescale_keep_original writes the input qualities
//              as OQ:Z on every record whose QUAL changed; FILE: the summary and the 64 bins of new qualities.  With --devices every device rescales its own reads)
//             [--pileup FILE [--pileup_unique] [--pileup_min_bq N] [--pileup_mask5 N] [--pileup_mask3 N] (A/C/G/T counts per reference position of the reported alignments, counted
//              on the GPU; per-contig statistics; same BAM)] [--consensus FASTA [--consensus_min_depth 1] [--consensus_min_percent 0] (the call of every position, N where there is none)]
//             [--allele_likelihoods FILE [--allele_unique] [--allele_min_bq N] [--allele_mask5 N] [--allele_mask3 N] (damage-aware consensus: per reference position the
//              log-likelihood of the reported alignments' columns under each allele A, C, G, T by the damage model -f/-t/-d/-s, summed on the GPU; per-contig statistics;
//              same BAM)] [--damage_consensus FASTA [--damage_consensus_min_depth 1] [--damage_consensus_min_margin 3.0] [--damage_consensus_qual FILE] (the most likely
//              allele where it leads the second by that many bits, N elsewhere; FILE: one line per contig, Phred+33 of min(margin in whole bits, 93))]
//             [--genotype_vcf FILE [--genotype_min_depth 1] [--genotype_min_margin 3.0] [--genotype_het_penalty 10.0] [--genotype_likelihoods TSV] (diploid genotype
//              likelihoods on top of the allele likelihoods — honours --allele_unique / --allele_min_bq / --allele_mask5 / --allele_mask3 —: VCF 4.2, one record per called
//              site whose genotype is not homozygous for the reference base of the -g FASTA; TSV: per-contig statistics; same BAM)]
//             [--snp_panel FILE.snp --panel_geno OUT.geno [--panel_snp OUT.snp] [--panel_ind OUT.ind [--panel_sample NAME] [--panel_population POP]] [--panel_counts OUT.tsv]
//              [--panel_call random|majority] [--panel_min_depth 1] [--panel_seed 0] [--panel_transitions keep|missing|single_strand] [--panel_unique] [--panel_min_bq N]
//              [--panel_mask5 N] [--panel_mask3 N] [--panel_report FILE] (pseudo-haploid genotypes at the rows of an EIGENSTRAT .snp file — id chrom genpos physpos ref alt —:
//              strand-split A/C/G/T counts at the panel's positions, counted on the GPU, and one call per row, 2 ref / 0 alt / 9 missing, in input order; single_strand uses
//              only reverse-strand reads at C/T rows and forward-strand reads at G/A rows; honours --exclude_duplicates, --damage_score_min and --rescale_pileup; with
//              --devices the tables are merged before the call; same BAM)]
//             [--reads2 R2.fastq[.gz] [--unmerged drop|single] | --trim_adapter] [--adapter1 SEQ] [--adapter2 SEQ] [--merge_min_overlap 11] [--trim_min_overlap 3]
//              [--merge_max_mismatch_permille 166] [--merge_min_length 15] [--merge_max_quality 41] [--merge_report FILE] (sequencer output in: the reader takes the same
//              number of records from -r and --reads2 per chunk, trims the adapters and merges each overlapping pair into one read on the first device — see `merge`
//              below —, and everything behind the reader maps the merged reads as ordinary single reads, flags 0, under mate 1's name without its /1.  Pairs that do
//              not merge are left out and counted, or with --unmerged single go on as two independent single reads NAME/1 and NAME/2, each trimmed with its own adapter;
//              pairs that merge to fewer than --merge_min_length bases are always left out.  --trim_adapter: single-end trimming of -r.  FASTQ only.  No pair flags are
//              set: this is not paired-end mapping)
//             [--trim_poly_g [--poly_min_length 10]] [--trim_ns] [--trim_qualities [--min_quality 2]] [--max_dust PERMILLE] [--clean_min_length 15] [--clean_report FILE]
//             (the read clean-up, on the first device, FASTQ only — see `clean` below: poly-G tails come off every read as sequenced, in front of the merger or adapter
//              trimmer if there is one; ends of N and of low-quality bases, the length test and the complexity filter run on the reads that go on to the mapper.  A read
//              left shorter than --clean_min_length or scoring above --max_dust is left out and counted.  Works without --reads2 or --trim_adapter as well)
//             [--gap_dist_ends 5] [--max_num_gaps_open 2] [--no_search_limit_recovery] [--force_overwrite] [-R ID]
//   mapad-amd analyse -g ref.fa --reads in.bam [--min_mapq N] [--original_qualities] [-o out.bam] [--analyse_report FILE] [every report / stage option of map, same names, same files]
//             [-l LIBRARY -f F -t T -d D -s S -D 0.02 (the damage model of the stages that score with it)] [--batch_size 250000]
//             (the accumulator stages over an existing BAM whose mapped records carry MD:Z — nothing is searched: each record's contig, POS, strand, CIGAR, MD, X0 and
//              AS become on the GPU what a search would have left there, and the stages count it; records of any status class but ok — unmapped, below --min_mapq, no MD,
//              soft-clipped, ... — are seen, not counted, and reported.  -o: the records as they are, in input order, with 0x400 under --mark_duplicates (dropped under
//              --exclude_duplicates) and QUAL, OQ:Z and DS:f written as map writes them.  --original_qualities: a record's OQ:Z, where it has one, is the quality the stages see
//              (for the BAM of map --rescale_keep_original).  BAM input only (no CRAM); the BAM's reference list must be the index's contigs; -f/-t/-d/-s are required by the
//              stages that score with the damage model.  One device)
//   mapad-amd merge -1 R1.fastq[.gz] [-2 R2.fastq[.gz]] -o OUT.fastq[.gz] [--host] [--adapter1 SEQ] [--adapter2 SEQ] [--merge_min_overlap 11] [--trim_min_overlap 3]
//             [--merge_max_mismatch_permille 166] [--merge_min_length 15] [--merge_max_quality 41] [--merge_report FILE] [--batch_size 250000]
//             (the step in front of mapping, alone: adapters trimmed and overlapping pairs merged into single reads on the GPU — merge_decide_kernel tries every
//              fragment length of a pair at once —, written as FASTQ under mate 1's name without its /1; pairs that do not merge, or merge to fewer than
//              --merge_min_length bases, are left out and counted.  With -1 alone: single-end adapter trimming, untouched reads written as they are.  --host: the same
//              rule on host threads, no GPU.  FILE: the counts by class, bases in and out, the mean length and the length histogram.  This is not paired-end mapping)
//             `merge` takes the clean-up options of `clean` too, placed as in `map`.
//   mapad-amd clean -1 R.fastq[.gz] -o OUT.fastq[.gz] [--host] [--trim_poly_g [--poly_min_length 10]] [--trim_ns] [--trim_qualities [--min_quality 2]] [--max_dust PERMILLE]
//             [--clean_min_length 15] [--clean_report FILE] [--batch_size 250000]
//             (the read clean-up alone, at least one op: a poly-G tail of >= 10 bases with at most one other base in eight cut off the 3' end; N and bases of quality
//              <= 2 removed from both ends; a read left shorter than 15 bases dropped; a read whose DUST-like score — 1000 for a homopolymer, about 20 for random
//              bases, 70 a usual threshold — exceeds PERMILLE dropped.  --host: the same rule on host threads, no GPU.  FILE: the counters, then the histograms of
//              output length and of the score)
//   mapad-amd mappability -g ref.fa [-k 35] [--max_mismatches 0|1] [--host] [--verify] [--bed FILE [--bed_rule start|majority|strict]] [--bedgraph FILE] [--report FILE] [--device N]
//             (at how many places of the reference — both strands, through the index the reads are mapped with — each of its k-mers occurs, exactly or with at most one
//              substitution, counted on the GPU contig by contig.  --bed: merged half-open runs of the positions in the chosen mask (start: the k-mer starting there is
//              unique; majority: more than half of the k-mers over the position are; strict: all of them; default majority), contig names as in the index; --bedgraph: the
//              start counts, saturated at 255, run-length encoded; --report: per-contig and total figures as TSV (a second pass over the reference).  --verify runs every
//              search to its end and stops if the FASTA is not the index's sequence.  --host: the same rule on host threads, no GPU, the same files)
//   mapad-amd panel -g ref.fa --snp_panel FILE.snp [-o OUT] (how map --snp_panel places the rows on the contigs: `id tid pos0` per row, tid -1 = unplaced; no GPU)
#include <algorithm>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mapad_amd.h"
#include "../mappability_core.hpp"  // the rule of the masks: possible_starts, mask_majority, mask_strict (host-compilable)
#include "../genotype_core.hpp"  // the pieces of the call rule that the VCF is written with: genotype_call, genotype_pl, genotype_allele (host-compilable)
#include "bam_io.hpp"
#include "wire.hpp"

#include <netdb.h>
#include <sys/socket.h>
#include <unistd.h>

using namespace mapad::cli;

namespace {

[[noreturn]] void die(const std::string& msg) { std::fprintf(stderr, "mapad-amd: %s\n", msg.c_str()); std::exit(1); }
void check(int rc, const char* what) { if (rc != MAPAD_OK) die(std::string(what) + " failed with status " + std::to_string(rc)); }

struct Args {
    std::map<std::string, std::string> kv;
    std::vector<std::string> flags;
    bool has(const std::string& k) const { return kv.count(k) != 0; }
    std::string get(const std::string& k, const std::string& d = "") const { auto it = kv.find(k); return it == kv.end() ? d : it->second; }
    float f(const std::string& k, float d) const { return has(k) ? std::strtof(kv.at(k).c_str(), nullptr) : d; }
    bool flag(const std::string& k) const { for (auto& f : flags) if (f == k) return true; return false; }
};

// FASTA -> contigs (names up to the first whitespace, like noodles' fasta record name)
void read_fasta(const std::string& path, std::vector<std::string>& names, std::vector<std::vector<uint8_t>>& seqs) {
    GzReader in(path);
    std::string line;
    while (in.getline(line)) {
        if (line.empty()) continue;
        if (line[0] == '>') {
            const size_t sp = line.find_first_of(" \t");
            names.push_back(line.substr(1, sp == std::string::npos ? std::string::npos : sp - 1));
            seqs.emplace_back();
        } else {
            if (seqs.empty()) die("FASTA does not start with '>'");
            seqs.back().insert(seqs.back().end(), line.begin(), line.end());
        }
    }
}

// create_bam_header (src/map/mapping.rs:300-398)
std::string make_header(const std::string& src, const mapad_index_t* idx, const std::string& read_group, const std::string& cmdline) {
    std::vector<std::string> pg, rg, co;
    std::string line;
    for (size_t i = 0; i <= src.size(); ++i) {
        if (i == src.size() || src[i] == '\n') {
            if (line.rfind("@PG", 0) == 0) pg.push_back(line);
            else if (line.rfind("@RG", 0) == 0) rg.push_back(line);
            else if (line.rfind("@CO", 0) == 0) co.push_back(line);
            line.clear();
        } else line.push_back(src[i]);
    }
    std::string out = "@HD\tVN:1.6\tSO:unsorted\n";
    for (uint32_t i = 0; i < mapad_index_n_contigs(idx); ++i) {
        const char* name; uint64_t s, e;
        check(mapad_index_contig(idx, i, &name, &s, &e), "mapad_index_contig");
        out += std::string("@SQ\tSN:") + name + "\tLN:" + std::to_string(e - s + 1) + "\n";
    }
    if (!read_group.empty()) out += "@RG\tID:" + read_group + "\n";
    else for (auto& l : rg) out += l + "\n";
    auto id_of = [](const std::string& l) { const size_t p = l.find("\tID:"); if (p == std::string::npos) return std::string(); const size_t e = l.find('\t', p + 4); return l.substr(p + 4, e == std::string::npos ? std::string::npos : e - p - 4); };
    size_t same = 0;
    std::string last_id;
    for (auto& l : pg) { out += l + "\n"; const std::string id = id_of(l); if (id == "mapAD" || id.rfind("mapAD.", 0) == 0) same += 1; last_id = id; }
    const std::string my_id = same ? "mapAD." + std::to_string(same) : "mapAD";
    out += "@PG\tID:" + my_id + "\tPN:mapAD\tVN:" + mapad_version() + "\tDS:An aDNA aware short-read mapper\tCL:" + cmdline + (last_id.empty() ? "" : "\tPP:" + last_id) + "\n";
    for (auto& l : co) out += l + "\n";
    return out;
}

int cmd_index(const Args& a, uint64_t seed, int device) {
    const std::string ref = a.get("reference");
    if (ref.empty()) die("index: -g/--reference is required");
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> seqs;
    read_fasta(ref, names, seqs);
    std::vector<const char*> np;
    std::vector<const uint8_t*> sp;
    std::vector<uint64_t> lens;
    for (size_t i = 0; i < names.size(); ++i) { np.push_back(names[i].c_str()); sp.push_back(seqs[i].data()); lens.push_back(seqs[i].size()); }
    mapad_index_t* idx = nullptr;
    // suffix sorting on the GPU when there is one (seconds for a 3 Gbp genome); the host SA-IS path builds the same files without a GPU
    int rc = a.flag("host_index") ? MAPAD_ERR_NO_DEVICE : mapad_index_build_gpu(np.data(), sp.data(), lens.data(), (uint32_t)names.size(), seed, device, &idx);
    if (rc == MAPAD_ERR_UNSUPPORTED || rc == MAPAD_ERR_NOMEM) {
        std::fprintf(stderr, "index: the GPU suffix sorter cannot take this text (%s); building on the host\n", rc == MAPAD_ERR_NOMEM ? "out of device memory" : "a prefix bucket or group beyond its limits");
        rc = MAPAD_ERR_NO_DEVICE;
    }
    if (rc == MAPAD_ERR_NO_DEVICE) rc = mapad_index_build(np.data(), sp.data(), lens.data(), (uint32_t)names.size(), seed, &idx);
    check(rc, "mapad_index_build");
    check(mapad_index_save(idx, ref.c_str()), "mapad_index_save");  // files are named <reference>.{tbw,...} (indexing.rs:110-208)
    mapad_index_free(idx);
    return 0;
}

// ---- `map`: a three-stage pipeline over chunks (run_inner's loop, src/map/mapping.rs:151-294) -------------------------------------------
//   reader  : parses the next chunk of input records into page-locked buffers
//   devices : one worker thread and one context per GPU; a chunk is cut into contiguous slices, one per device (the reference's rayon map over
//             the chunk, order-preserving, mapping.rs:153-156,288).  A worker submits its slice of chunk k + 1 before it collects chunk k, so the
//             GPU maps while the host turns the previous chunk's hits into records (SA locate on the same GPU, strings on host threads).
//   writer  : encodes and BGZF-compresses the records of a finished chunk on several threads, writes them in input order.
// Results reach the writer through page-locked host memory, each GPU over its own PCIe link; there is no GPU-to-GPU hop in a single process.
template <class T>
class BoundedQueue {
public:
    explicit BoundedQueue(size_t cap) : cap_(cap) {}
    void push(T v) {
        std::unique_lock<std::mutex> l(mu_);
        not_full_.wait(l, [&] { return q_.size() < cap_; });
        q_.push_back(std::move(v));
        not_empty_.notify_all();
    }
    bool pop(T& out) {  // false: closed and drained
        std::unique_lock<std::mutex> l(mu_);
        not_empty_.wait(l, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        not_full_.notify_all();
        return true;
    }
    void close() { std::lock_guard<std::mutex> l(mu_); closed_ = true; not_empty_.notify_all(); }
private:
    size_t cap_;
    std::deque<T> q_;
    std::mutex mu_;
    std::condition_variable not_full_, not_empty_;
    bool closed_ = false;
};

struct PinnedBytes {  // page-locked byte buffer from the library (DMA at link speed)
    uint8_t* p = nullptr;
    size_t n = 0, cap = 0;
    void append(const void* src, size_t k) {
        if (n + k > cap) {
            const size_t want = std::max<size_t>((n + k) * 2, 1 << 20);
            uint8_t* q = (uint8_t*)mapad_host_alloc(want);
            if (!q) die("out of page-locked host memory");
            if (n) std::memcpy(q, p, n);
            mapad_host_free(p);
            p = q; cap = want;
        }
        if (k) std::memcpy(p + n, src, k);
        n += k;
    }
    void resize_uninitialized(size_t k) {  // contents are written by the caller
        if (k > cap) { n = 0; append(nullptr, 0); const size_t want = std::max<size_t>(k * 2, 1 << 20); uint8_t* q = (uint8_t*)mapad_host_alloc(want); if (!q) die("out of page-locked host memory"); mapad_host_free(p); p = q; cap = want; }
        n = k;
    }
    ~PinnedBytes() { mapad_host_free(p); }
};

struct Slice {
    uint64_t lo = 0, hi = 0;  // reads [lo, hi) of the chunk's mappable reads
    std::vector<uint64_t> offsets;  // rebased to the slice
    mapad_batch_result_t* res = nullptr;
    mapad_coords_t* coords = nullptr;  // device half of the records (mapad_hits_to_coords_gpu), consumed by the records thread
    mapad_records_t* recs = nullptr;
};
struct Chunk {
    uint64_t no = 0;
    uint64_t first_read = 0;         // mapped reads of the run before this chunk: read k of the chunk is read first_read + k of the run (the records' seeds count in reads of the run)
    std::vector<InRecord> in;        // every input record, in input order
    std::vector<int64_t> read_of;    // per input record: its index among the mapped reads, -1 if it cannot be mapped (empty / longer than the device limit)
    PinnedBytes seqs, quals;         // mapped reads, concatenated
    std::vector<uint64_t> offsets;
    std::vector<uint16_t> flags;
    std::vector<Slice> slices;
    std::atomic<int> pending{0};
    std::chrono::steady_clock::time_point t_submit;
    float per_read_s = 0.0f;
};
using ChunkPtr = std::shared_ptr<Chunk>;

std::vector<int> parse_devices(const std::string& spec) {  // "0", "0,2,3", "0-7"
    std::vector<int> out;
    size_t i = 0;
    while (i < spec.size()) {
        size_t j = i;
        while (j < spec.size() && spec[j] != ',') ++j;
        const std::string tok = spec.substr(i, j - i);
        const size_t dash = tok.find('-');
        if (dash != std::string::npos && dash > 0) { for (int d = std::atoi(tok.substr(0, dash).c_str()); d <= std::atoi(tok.substr(dash + 1).c_str()); ++d) out.push_back(d); }
        else if (!tok.empty()) out.push_back(std::atoi(tok.c_str()));
        i = j + 1;
    }
    if (out.empty()) die("--devices: empty device list");
    return out;
}

void parallel_for(size_t n, unsigned threads, const std::function<void(size_t, size_t, unsigned)>& fn) {  // contiguous ranges
    threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n));
    if (threads == 1) { fn(0, n, 0); return; }
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t) pool.emplace_back([&, t] { fn(n * t / threads, n * (t + 1) / threads, t); });
    for (auto& th : pool) th.join();
}

// An EIGENSTRAT .snp file: per line `id chrom genpos physpos ref alt`, whitespace-separated, physpos 1-based; its rows placed on the index's contigs.  A
// chromosome names a contig by, in this order: its exact name; "chr" + name; 23 / 24 / 90 as X / Y / MT, also with "chr", and chrM for 90.  A row whose
// chromosome names no contig (or whose position is 0) is unplaced — tid -1 —, not an error; a malformed line is one, named by its number.
struct SnpPanelFile {
    std::vector<std::string> lines, id, chrom;  // the lines as read (copied by --panel_snp)
    std::vector<int32_t> tid;
    std::vector<uint64_t> pos0, physpos;
    std::vector<uint8_t> ref, alt;
};
int32_t panel_contig_of(const std::map<std::string, int32_t>& contigs, const std::string& chrom) {
    std::vector<std::string> names = {chrom, "chr" + chrom};
    const char* alias = chrom == "23" ? "X" : chrom == "24" ? "Y" : chrom == "90" ? "MT" : nullptr;
    if (alias) { names.push_back(alias); names.push_back(std::string("chr") + alias); }
    if (chrom == "90") names.push_back("chrM");
    for (const auto& n : names) { auto it = contigs.find(n); if (it != contigs.end()) return it->second; }
    return -1;
}
SnpPanelFile read_snp_panel(const std::string& path, const mapad_index_t* idx) {
    std::map<std::string, int32_t> contigs;
    for (uint32_t t = 0; t < mapad_index_n_contigs(idx); ++t) {
        const char* name; uint64_t s, e;
        check(mapad_index_contig(idx, t, &name, &s, &e), "mapad_index_contig");
        contigs.emplace(name, (int32_t)t);
    }
    std::ifstream in(path);
    if (!in) die("cannot read " + path);
    SnpPanelFile P;
    std::string line;
    for (uint64_t n = 1; std::getline(in, line); ++n) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::istringstream f(line);
        std::vector<std::string> w;
        for (std::string t; f >> t;) w.push_back(t);
        if (w.empty()) continue;  // a blank line is no row
        const auto bad = [&](const char* why) { die(path + ": line " + std::to_string(n) + ": " + why); };
        if (w.size() != 6) bad("expected 6 fields: id chrom genpos physpos ref alt");
        char* end = nullptr;
        (void)std::strtod(w[2].c_str(), &end);
        if (end == w[2].c_str() || *end) bad("the genetic position is not a number");
        if (w[3].empty() || w[3].find_first_not_of("0123456789") != std::string::npos || w[3].size() > 18) bad("the physical position is not a non-negative integer");
        if (w[4].size() != 1 || w[5].size() != 1) bad("ref and alt are one character each");
        const uint64_t phys = std::strtoull(w[3].c_str(), nullptr, 10);
        P.lines.push_back(line); P.id.push_back(w[0]); P.chrom.push_back(w[1]); P.physpos.push_back(phys);
        P.tid.push_back(phys ? panel_contig_of(contigs, w[1]) : -1); P.pos0.push_back(phys ? phys - 1 : 0);
        P.ref.push_back((uint8_t)w[4][0]); P.alt.push_back((uint8_t)w[5][0]);
    }
    if (P.lines.empty()) die(path + ": no panel rows");
    return P;
}
void write_lines(const std::string& path, const std::function<void(FILE*)>& body) {
    FILE* f = std::fopen(path.c_str(), "w");
    if (!f) die("cannot write " + path);
    body(f);
    if (std::fclose(f) != 0) die("cannot write " + path);
}
// `mapad-amd panel -g REF --snp_panel FILE.snp [-o OUT]`: the panel's rows as `map --snp_panel` places them, one line `id tid pos0` each (tid -1: unplaced); no GPU
int cmd_panel(const Args& a) {
    if (!a.has("reference") || !a.has("snp_panel")) die("panel: --reference and --snp_panel are required");
    mapad_index_t* idx = nullptr;
    check(mapad_index_open(a.get("reference").c_str(), &idx), "mapad_index_open");
    const SnpPanelFile P = read_snp_panel(a.get("snp_panel"), idx);
    FILE* f = a.has("output") ? std::fopen(a.get("output").c_str(), "w") : stdout;
    if (!f) die("cannot write " + a.get("output"));
    for (size_t i = 0; i < P.id.size(); ++i) std::fprintf(f, "%s\t%d\t%llu\n", P.id[i].c_str(), P.tid[i], (unsigned long long)P.pos0[i]);
    if (f != stdout && std::fclose(f) != 0) die("cannot write " + a.get("output"));
    mapad_index_free(idx);
    return 0;
}

// ---- `mapad-amd mappability`: loci of every reference k-mer through the mapper's own index, contig by contig -------------------------------------------------
int cmd_mappability(const Args& a, int device) {
    namespace mp = mapad::mappability;
    if (!a.has("reference")) die("mappability: -g/--reference is required");
    const long k = std::strtol(a.get("k", "35").c_str(), nullptr, 10), e = std::strtol(a.get("max_mismatches", "0").c_str(), nullptr, 10);
    if (k < 1 || k > mp::kMaxK) die("mappability: -k must be in 1..255");
    if (e < 0 || e > 1) die("mappability: --max_mismatches must be 0 or 1");
    const std::string rule = a.get("bed_rule", "majority");
    if (rule != "start" && rule != "majority" && rule != "strict") die("mappability: --bed_rule must be start, majority or strict");
    const bool host = a.flag("host");
    const uint32_t flags = a.flag("verify") ? MAPAD_MAPPABILITY_VERIFY : 0u;
    std::vector<std::string> names;
    std::vector<std::vector<uint8_t>> seqs;
    read_fasta(a.get("reference"), names, seqs);
    mapad_index_t* idx = nullptr;
    check(mapad_index_open(a.get("reference").c_str(), &idx), "mapad_index_open");
    const uint32_t nc = mapad_index_n_contigs(idx);
    if (nc != names.size()) die("mappability: the FASTA and the index differ in their number of contigs");
    std::vector<std::string> idx_names;
    for (uint32_t i = 0; i < nc; ++i) {
        const char* name; uint64_t s, en;
        check(mapad_index_contig(idx, i, &name, &s, &en), "mapad_index_contig");
        if (en - s + 1 != seqs[i].size()) die("mappability: contig " + names[i] + " of the FASTA has another length than contig " + name + " of the index");
        idx_names.push_back(name);
    }
    mapad_ctx_t* ctx = nullptr;
    if (!host) {  // (the search's settings are not used: nothing is aligned)
        mapad_params_t prm;
        check(mapad_params_from_cli(&prm, MAPAD_LIBRARY_SINGLE_STRANDED, 0, 0, 0, 0, 0.02f, 0.03f, 0, 1.0f, 0.001f, 1.0f, 5, 2, 0, 0, 250000), "mapad_params_from_cli");
        check(mapad_ctx_create(idx, &prm, device, &ctx), "mapad_ctx_create");
    }
    auto open_out = [&](const char* key) -> FILE* {
        if (!a.has(key)) return nullptr;
        FILE* f = std::fopen(a.get(key).c_str(), "w");
        if (!f) die("cannot write " + a.get(key));
        return f;
    };
    FILE* bed = open_out("bed");
    FILE* bedgraph = open_out("bedgraph");
    std::vector<uint8_t> counts, cover;
    for (uint32_t i = 0; i < nc && (bed || bedgraph); ++i) {
        const uint64_t len = seqs[i].size();
        counts.assign(len, 0); cover.assign(len, 0);
        const int rc = host ? mapad_mappability_host(idx, i, seqs[i].data(), len, 0, len, (uint32_t)k, (uint32_t)e, flags, counts.data(), cover.data())
                            : mapad_ctx_mappability(ctx, i, seqs[i].data(), len, 0, len, (uint32_t)k, (uint32_t)e, flags, counts.data(), cover.data());
        if (rc == MAPAD_ERR_INVALID && flags) die("mappability: --verify: contig " + names[i] + " of the FASTA is not the sequence the index was built from");
        check(rc, "mapad_mappability");
        const char* name = idx_names[i].c_str();
        if (bed) {  // merged half-open runs of the chosen mask
            uint64_t run = 0;
            bool in = false;
            for (uint64_t x = 0; x <= len; ++x) {
                bool m = false;
                if (x < len) {
                    const uint32_t possible = mp::possible_starts(x, (uint32_t)k, len);
                    m = rule == "start" ? counts[x] == 1 : rule == "majority" ? mp::mask_majority(cover[x], possible) : mp::mask_strict(cover[x], possible);
                }
                if (m && !in) { run = x; in = true; }
                else if (!m && in) { std::fprintf(bed, "%s\t%llu\t%llu\n", name, (unsigned long long)run, (unsigned long long)x); in = false; }
            }
        }
        if (bedgraph)  // the start counts, run-length encoded
            for (uint64_t x = 0, run = 0; x <= len; ++x)
                if (x == len || counts[x] != counts[run]) {
                    if (x > run) std::fprintf(bedgraph, "%s\t%llu\t%llu\t%u\n", name, (unsigned long long)run, (unsigned long long)x, (unsigned)counts[run]);
                    run = x;
                }
    }
    for (FILE* f : {bed, bedgraph}) if (f && std::fclose(f) != 0) die("mappability: cannot write an output file");
    if (a.has("report")) {
        std::vector<const uint8_t*> sp;
        std::vector<uint64_t> lens;
        for (auto& s : seqs) { sp.push_back(s.data()); lens.push_back(s.size()); }
        std::vector<mapad_mappability_contig_t> rows(nc);
        mapad_mappability_t sum{};
        sum.n_contigs = nc; sum.contigs = rows.data();
        const int rc = host ? mapad_mappability_summary_host(idx, sp.data(), lens.data(), (uint32_t)k, (uint32_t)e, flags, &sum)
                            : mapad_ctx_mappability_summary(ctx, sp.data(), lens.data(), (uint32_t)k, (uint32_t)e, flags, &sum);
        if (rc == MAPAD_ERR_INVALID && flags) die("mappability: --verify: the FASTA is not the sequence the index was built from");
        check(rc, "mapad_mappability_summary");
        FILE* f = open_out("report");
        std::fprintf(f, "#k\t%ld\n#max_mismatches\t%ld\n", k, e);
        std::fprintf(f, "contig\tlength\tvalid_starts\tunique_starts\tc1\tc2\tc3_4\tc5_8\tc9_16\tc17_32\tc33_64\tc65_128\tc129_up\tmajority\tstrict\n");
        auto row = [&](const char* name, const mapad_mappability_contig_t& r) {
            std::fprintf(f, "%s\t%llu\t%llu\t%llu", name, (unsigned long long)r.length, (unsigned long long)r.valid_starts, (unsigned long long)r.unique_starts);
            for (int b = 0; b < MAPAD_MAPPABILITY_BINS; ++b) std::fprintf(f, "\t%llu", (unsigned long long)r.hist[b]);
            std::fprintf(f, "\t%llu\t%llu\n", (unsigned long long)r.majority, (unsigned long long)r.strict);
        };
        for (uint32_t i = 0; i < nc; ++i) row(idx_names[i].c_str(), rows[i]);
        row("total", sum.total);
        if (std::fclose(f) != 0) die("cannot write " + a.get("report"));
    }
    if (ctx) mapad_ctx_destroy(ctx);
    mapad_index_free(idx);
    return 0;
}

// ---- `mapad-amd merge`: adapter trimming and read-pair merging alone, FASTQ in, FASTQ out ------------------------------------------------------------------
mapad_merge_params_t merge_params_from(const Args& a, uint32_t mode) {
    mapad_merge_params_t p;
    mapad_merge_params_default(&p);
    p.mode = mode;
    auto num = [&](const char* key, uint32_t& v) { if (a.has(key)) v = (uint32_t)std::strtoul(a.get(key).c_str(), nullptr, 10); };
    num("merge_min_overlap", p.min_overlap); num("trim_min_overlap", p.min_adapter_overlap); num("merge_max_mismatch_permille", p.max_mismatch_permille);
    num("merge_min_length", p.min_length); num("merge_max_quality", p.max_quality);
    auto adapter = [&](const char* key, uint8_t* dst, uint32_t& len) {
        if (!a.has(key)) return;
        std::string s = a.get(key);
        for (auto& c : s) c = (char)std::toupper((unsigned char)c);
        if (s.size() > MAPAD_MERGE_MAX_ADAPTER) die(std::string("--") + key + ": an adapter may have at most 64 bases");
        len = (uint32_t)s.size();
        std::memset(dst, 0, MAPAD_MERGE_MAX_ADAPTER);
        std::memcpy(dst, s.data(), s.size());
    };
    adapter("adapter1", p.adapter1, p.adapter1_len); adapter("adapter2", p.adapter2, p.adapter2_len);
    if (mapad_merge_params_check(&p) != MAPAD_OK)
        die("merge: adapters of at most 64 bases A, C, G, T; --merge_min_overlap and --trim_min_overlap >= 1; --merge_max_quality <= 93; --merge_max_mismatch_permille <= 1000");
    return p;
}
std::string mate_base_name(const std::string& name, char mate) {  // NAME/1 -> NAME
    const size_t n = name.size();
    return (n >= 2 && name[n - 2] == '/' && name[n - 1] == mate) ? name.substr(0, n - 2) : name;
}
struct PackedReads {
    std::vector<uint8_t> seqs, quals;
    std::vector<uint64_t> offsets{0};
    void add(const InRecord& r) {
        seqs.insert(seqs.end(), r.seq.begin(), r.seq.end());
        if (r.qual.size() == r.seq.size()) quals.insert(quals.end(), r.qual.begin(), r.qual.end());
        else quals.insert(quals.end(), r.seq.size(), (uint8_t)255);
        offsets.push_back(seqs.size());
    }
    void clear() { seqs.clear(); quals.clear(); offsets.assign(1, 0); }
};
// `key\tvalue` lines, then `length\tcount` lines of the histogram's non-empty bins
void write_merge_report(const std::string& path, const mapad_merge_counts_t& c, bool single) {
    static const char* pair_names[] = {"merged", "too_short", "unmerged", "empty_mate", "too_long"};
    static const char* single_names[] = {"trimmed", "too_short", "untouched", "empty_mate", "too_long"};
    write_lines(path, [&](FILE* f) {
        std::fprintf(f, "%s\t%llu\n", single ? "reads_seen" : "pairs_seen", (unsigned long long)c.pairs_seen);
        for (int k = 0; k < MAPAD_MERGE_CLASSES; ++k) std::fprintf(f, "%s\t%llu\n", (single ? single_names : pair_names)[k], (unsigned long long)c.class_counts[k]);
        std::fprintf(f, "bases_in\t%llu\nbases_out\t%llu\n", (unsigned long long)c.bases_in, (unsigned long long)c.bases_out);
        uint64_t n = 0, sum = 0;
        for (int k = 0; k < MAPAD_MERGE_HIST_BINS; ++k) { n += c.histogram[k]; sum += c.histogram[k] * (uint64_t)k; }
        std::fprintf(f, "mean_length\t%.3f\n", n ? (double)sum / (double)n : 0.0);
        for (int k = 0; k < MAPAD_MERGE_HIST_BINS; ++k) if (c.histogram[k]) std::fprintf(f, "%d\t%llu\n", k, (unsigned long long)c.histogram[k]);
    });
}
// ---- the read clean-up (--trim_poly_g, --trim_ns, --trim_qualities, --max_dust) as `clean`, `merge` and the reader of `map` run it -----------------------------
// Two passes when a merge stage stands between them (`split`): the poly-G tails come off every read as sequenced, before the merger sees it (no read is dropped
// there: the files stay in step); the ends, the length test and the complexity filter run on the reads that go on to the mapper.  Without a merge stage one
// pass does all of it.  A dropped read is left out of the chunk and counted.
struct CleanStage {
    bool host, split;
    bool on_front = false, on_back = false;
    mapad_clean_params_t front_params{}, back_params{};
    mapad_cleaner_t *front_cleaner = nullptr, *back_cleaner = nullptr;
    mapad_clean_counts_t front_total{}, back_total{};
    uint64_t reads_written = 0;
    static bool wanted(const Args& a) { return a.flag("trim_poly_g") || a.flag("trim_ns") || a.flag("trim_qualities") || a.has("max_dust"); }
    // an option that depends on another, or all of them with no op at all, is refused rather than ignored
    static void check_options(const Args& a, const std::string& cmd) {
        if (a.has("poly_min_length") && !a.flag("trim_poly_g")) die(cmd + ": --poly_min_length does nothing without --trim_poly_g");
        if (a.has("min_quality") && !a.flag("trim_qualities")) die(cmd + ": --min_quality does nothing without --trim_qualities");
        if (!wanted(a))
            for (const char* k : {"clean_min_length", "clean_report"})
                if (a.has(k)) die(cmd + ": --" + k + " does nothing without --trim_poly_g, --trim_ns, --trim_qualities or --max_dust (no read is cleaned)");
    }
    CleanStage(const Args& a, int device, bool host_, bool split_, const std::string& cmd) : host(host_), split(split_) {
        mapad_clean_params_t p;
        mapad_clean_params_default(&p);
        auto num = [&](const char* key, uint32_t& v) {
            if (!a.has(key)) return;
            char* end = nullptr;
            const std::string s = a.get(key);
            const unsigned long long x = std::strtoull(s.c_str(), &end, 10);
            if (s.empty() || *end || s[0] == '-' || x > 0xFFFFFFFFull) die(cmd + ": --" + key + " takes a number");
            v = (uint32_t)x;
        };
        num("poly_min_length", p.poly_min_len); num("min_quality", p.min_quality); num("clean_min_length", p.min_length); num("max_dust", p.max_dust);
        const uint32_t poly = a.flag("trim_poly_g") ? MAPAD_CLEAN_POLY : 0u;
        const uint32_t rest = (a.flag("trim_ns") ? MAPAD_CLEAN_TRIM_N : 0u) | (a.flag("trim_qualities") ? MAPAD_CLEAN_TRIM_QUAL : 0u) | (a.has("max_dust") ? MAPAD_CLEAN_DUST : 0u);
        front_params = back_params = p;
        if (split) {
            front_params.ops = poly; front_params.min_length = 0;
            back_params.ops = rest;
            on_front = poly != 0; on_back = rest != 0 || a.has("clean_min_length");
        } else {
            back_params.ops = poly | rest;
            on_back = true;
        }
        if (mapad_clean_params_check(&front_params) != MAPAD_OK || mapad_clean_params_check(&back_params) != MAPAD_OK)
            die(cmd + ": --poly_min_length >= 1; --min_quality <= 93; --max_dust <= 1000 (permille)");
        if (!host) {
            if (on_front) check(mapad_cleaner_create(device, &front_params, &front_cleaner), "mapad_cleaner_create");
            if (on_back) check(mapad_cleaner_create(device, &back_params, &back_cleaner), "mapad_cleaner_create");
        }
    }
    CleanStage(const CleanStage&) = delete;
    ~CleanStage() { mapad_cleaner_free(front_cleaner); mapad_cleaner_free(back_cleaner); }
    mapad_clean_result_t* run(const mapad_clean_params_t& P, mapad_cleaner_t* c, mapad_clean_counts_t& total, const PackedReads& p) {
        mapad_clean_result_t* res = nullptr;
        const uint64_t n = p.offsets.size() - 1;
        check(host ? mapad_clean_reads_host(&P, p.seqs.data(), p.quals.data(), p.offsets.data(), n, &res) : mapad_clean_reads(c, p.seqs.data(), p.quals.data(), p.offsets.data(), n, &res),
              "mapad_clean_reads");
        mapad_clean_counts_add(&total, &res->counts);
        return res;
    }
    // the reads as sequenced, in front of the merger: every read keeps its slot (a read that is all tail becomes an empty one)
    void front(PackedReads& p) {
        if (!on_front || p.offsets.size() < 2) return;
        mapad_clean_result_t* res = run(front_params, front_cleaner, front_total, p);
        p.seqs.assign(res->seqs, res->seqs + res->total_bases);
        p.quals.assign(res->quals, res->quals + res->total_bases);
        p.offsets.assign(res->offsets, res->offsets + res->n_reads + 1);
        mapad_clean_result_free(res);
    }
    // the reads that go on to the mapper: trimmed in place, the dropped ones left out
    void back(std::vector<InRecord>& reads) {
        if (!on_back || reads.empty()) { reads_written += reads.size(); return; }
        PackedReads p;
        for (const InRecord& r : reads) p.add(r);
        mapad_clean_result_t* res = run(back_params, back_cleaner, back_total, p);
        size_t kept = 0;
        for (size_t i = 0; i < reads.size(); ++i) {
            const uint8_t cls = res->cls[i];
            if (cls != 0 && cls != 1 && cls != 5) continue;  // the classes that yield a read
            InRecord& r = reads[i];
            if (cls == 1) {
                const uint64_t b = res->offsets[i], len = res->offsets[i + 1] - b;
                const bool has_qual = r.qual.size() == r.seq.size();
                r.seq.assign((const char*)res->seqs + b, len);
                if (has_qual) r.qual.assign(res->quals + b, res->quals + b + len);
            }
            if (kept != i) reads[kept] = std::move(r);
            ++kept;
        }
        reads.resize(kept);
        reads_written += kept;
        mapad_clean_result_free(res);
    }
    // the stage alone in front of the mapper or of `clean`'s writer: up to max_records records from the input; false once the input has ended
    bool next_chunk(ReadSource& in, size_t max_records, std::vector<InRecord>& out) {
        InRecord r;
        bool more = true;
        while (out.size() < max_records && (more = in.next(r))) out.push_back(std::move(r));
        back(out);
        return more;
    }
    // `key\tvalue` lines of the counters, then `length_histogram\tBINS` and that many `length\tcount` lines, then `dust_histogram\tBINS` and `dust\tcount` lines
    // (dust: the bin's first permille).  The counters are those of the pass over the reads that go on; a poly-G pass in front of a merger adds its mates_* lines
    void report(const Args& a, const std::string& cmd) const {
        static const char* names[] = {"kept", "trimmed", "too_short", "low_complexity", "empty", "too_long"};
        const bool both = on_front && on_back;
        const mapad_clean_counts_t& c = on_back ? back_total : front_total;
        if (a.has("clean_report"))
            write_lines(a.get("clean_report"), [&](FILE* f) {
                std::fprintf(f, "reads_seen\t%llu\n", (unsigned long long)c.reads_seen);
                for (int k = 0; k < MAPAD_CLEAN_CLASSES; ++k) std::fprintf(f, "%s\t%llu\n", names[k], (unsigned long long)c.class_counts[k]);
                std::fprintf(f, "bases_in\t%llu\nbases_out\t%llu\nbases_poly\t%llu\nbases_trim5\t%llu\nbases_trim3\t%llu\n", (unsigned long long)c.bases_in, (unsigned long long)c.bases_out,
                             (unsigned long long)c.bases_poly, (unsigned long long)c.bases_trim5, (unsigned long long)c.bases_trim3);
                if (both)
                    std::fprintf(f, "mates_seen\t%llu\nmates_trimmed\t%llu\nmates_bases_in\t%llu\nmates_bases_poly\t%llu\n", (unsigned long long)front_total.reads_seen,
                                 (unsigned long long)front_total.class_counts[1], (unsigned long long)front_total.bases_in, (unsigned long long)front_total.bases_poly);
                int bins = 0;
                for (int k = 0; k < MAPAD_CLEAN_LEN_BINS; ++k) bins += c.length_histogram[k] != 0;
                std::fprintf(f, "length_histogram\t%d\n", bins);
                for (int k = 0; k < MAPAD_CLEAN_LEN_BINS; ++k) if (c.length_histogram[k]) std::fprintf(f, "%d\t%llu\n", k, (unsigned long long)c.length_histogram[k]);
                bins = 0;
                for (int k = 0; k < MAPAD_CLEAN_DUST_BINS; ++k) bins += c.dust_histogram[k] != 0;
                std::fprintf(f, "dust_histogram\t%d\n", bins);
                for (int k = 0; k < MAPAD_CLEAN_DUST_BINS; ++k) if (c.dust_histogram[k]) std::fprintf(f, "%d\t%llu\n", 10 * k, (unsigned long long)c.dust_histogram[k]);
            });
        std::fprintf(stderr, "%s: clean-up: %llu reads seen, %llu trimmed, %llu too short, %llu of low complexity; %llu bases in, %llu out", cmd.c_str(), (unsigned long long)c.reads_seen,
                     (unsigned long long)c.class_counts[1], (unsigned long long)c.class_counts[2], (unsigned long long)c.class_counts[3], (unsigned long long)c.bases_in,
                     (unsigned long long)c.bases_out);
        if (both) std::fprintf(stderr, "; %llu of %llu mates lost a poly-G tail (%llu bases)", (unsigned long long)front_total.class_counts[1], (unsigned long long)front_total.reads_seen,
                               (unsigned long long)front_total.bases_poly);
        std::fprintf(stderr, "\n");
    }
};

// The stage as `merge` and the reader of `map` run it: records of one file (single-end trimming) or of two files in step (pairs) in, the reads they yield out.
// Pairs: a merged pair is one read under mate 1's name without its /1.  `unmerged_single`: both mates of a pair of class 2 to 4 go on as independent single
// reads NAME/1 and NAME/2, each trimmed by the single-end rule with its own adapter (dropped when fewer than min_length bases are left; a mate too long for the
// rule goes on as it is).  Errors (the files end at different records, a pair's names differ) are exceptions that name the record.
struct MergeStage {
    bool single, host, unmerged_single;
    std::string path1, path2;
    mapad_merge_params_t P, T1, T2;  // the run's mode; mate 1 alone; mate 2 alone (adapter 2 in adapter 1's place)
    mapad_merger_t *M = nullptr, *M1 = nullptr, *M2 = nullptr;
    std::unique_ptr<ReadSource> in2;
    mapad_merge_counts_t total{};
    uint64_t record = 0, singles_written = 0, singles_dropped = 0, reads_written = 0;
    CleanStage* clean = nullptr;  // the clean-up around this stage, if any: poly-G tails off the mates in front of it, the rest on the reads it yields
    MergeStage(const Args& a, int device, bool host_, const std::string& reads1, const std::string& reads2)
        : single(reads2.empty()), host(host_), unmerged_single(a.get("unmerged", "drop") == "single"), path1(reads1), path2(reads2) {
        if (a.has("unmerged") && a.get("unmerged") != "drop" && a.get("unmerged") != "single") die("--unmerged takes drop or single");
        if (single && a.has("unmerged")) die("--unmerged says what becomes of pairs that do not merge and needs two files");
        P = merge_params_from(a, single ? 1u : 0u);
        T1 = P; T1.mode = 1;
        T2 = T1; T2.adapter1_len = P.adapter2_len; std::memcpy(T2.adapter1, P.adapter2, MAPAD_MERGE_MAX_ADAPTER);
        if (!single) in2.reset(new ReadSource(reads2));
        if (in2 && in2->is_bam()) die("--reads2: FASTQ input only (BAM and CRAM pairs are not supported)");
        if (!host) {
            check(mapad_merger_create(device, &P, &M), "mapad_merger_create");
            if (!single && unmerged_single) { check(mapad_merger_create(device, &T1, &M1), "mapad_merger_create"); check(mapad_merger_create(device, &T2, &M2), "mapad_merger_create"); }
        }
    }
    MergeStage(const MergeStage&) = delete;
    ~MergeStage() { mapad_merger_free(M); mapad_merger_free(M1); mapad_merger_free(M2); }
    mapad_merge_result_t* trim(const mapad_merge_params_t& T, mapad_merger_t* m, const PackedReads& p) {
        mapad_merge_result_t* res = nullptr;
        const uint64_t n = p.offsets.size() - 1;
        check(host ? mapad_trim_reads_host(&T, p.seqs.data(), p.quals.data(), p.offsets.data(), n, &res) : mapad_trim_reads(m, p.seqs.data(), p.quals.data(), p.offsets.data(), n, &res),
              "mapad_trim_reads");
        return res;
    }
    static InRecord record_of(const std::string& name, const uint8_t* seq, const uint8_t* qual, uint64_t len) {
        InRecord r;
        r.name = name; r.has_name = true; r.flags = 0;
        r.seq.assign((const char*)seq, len);
        r.qual.assign(qual, qual + len);
        return r;
    }
    // up to max_records records (pairs) from the input; false once the input has ended
    bool next_chunk(ReadSource& in1, size_t max_records, std::vector<InRecord>& out) {
        PackedReads p1, p2;
        std::vector<std::string> names;
        InRecord r1, r2;
        bool more = true;
        while (names.size() < max_records) {
            const bool got1 = in1.next(r1), got2 = single ? got1 : in2->next(r2);
            if (got1 != got2) throw std::runtime_error((got1 ? path2 : path1) + " ends at record " + std::to_string(record + 1) + " while the other file goes on");
            if (!got1) { more = false; break; }
            ++record;
            const std::string name = single ? r1.name : mate_base_name(r1.name, '1');
            if (!single && name != mate_base_name(r2.name, '2')) throw std::runtime_error("the names of record " + std::to_string(record) + " differ: " + r1.name + " and " + r2.name);
            names.push_back(name);
            p1.add(r1);
            if (!single) p2.add(r2);
        }
        const uint64_t n = names.size();
        if (!n) return more;
        if (clean) { clean->front(p1); if (!single) clean->front(p2); }
        mapad_merge_result_t* res = nullptr;
        if (single) res = trim(P, M, p1);
        else check(host ? mapad_merge_pairs_host(&P, p1.seqs.data(), p1.quals.data(), p1.offsets.data(), p2.seqs.data(), p2.quals.data(), p2.offsets.data(), n, &res)
                        : mapad_merge_pairs(M, p1.seqs.data(), p1.quals.data(), p1.offsets.data(), p2.seqs.data(), p2.quals.data(), p2.offsets.data(), n, &res), "mapad_merge_pairs");
        mapad_merge_counts_add(&total, &res->counts);
        // the mates that go on alone, trimmed
        PackedReads u1, u2;
        mapad_merge_result_t *t1 = nullptr, *t2 = nullptr;
        if (!single && unmerged_single) {
            auto take = [](PackedReads& dst, const PackedReads& src, uint64_t i) {
                const uint64_t b = src.offsets[i], e = src.offsets[i + 1];
                dst.seqs.insert(dst.seqs.end(), src.seqs.begin() + b, src.seqs.begin() + e); dst.quals.insert(dst.quals.end(), src.quals.begin() + b, src.quals.begin() + e);
                dst.offsets.push_back(dst.seqs.size());
            };
            for (uint64_t i = 0; i < n; ++i) if (res->cls[i] >= 2) { take(u1, p1, i); take(u2, p2, i); }
            if (u1.offsets.size() > 1) { t1 = trim(T1, M1, u1); t2 = trim(T2, M2, u2); }
        }
        uint64_t u = 0;
        auto alone = [&](const mapad_merge_result_t* t, const PackedReads& mate, uint64_t k, const std::string& name) {
            if (t->cls[k] == 0 || t->cls[k] == 2) out.push_back(record_of(name, t->seqs + t->offsets[k], t->quals + t->offsets[k], t->offsets[k + 1] - t->offsets[k]));
            else if (t->cls[k] == 4) out.push_back(record_of(name, mate.seqs.data() + mate.offsets[k], mate.quals.data() + mate.offsets[k], mate.offsets[k + 1] - mate.offsets[k]));
            else { ++singles_dropped; return; }
            ++singles_written;
        };
        for (uint64_t i = 0; i < n; ++i) {
            if (res->cls[i] == 0 || (single && res->cls[i] == 2)) {  // the classes that yield a read
                out.push_back(record_of(names[i], res->seqs + res->offsets[i], res->quals + res->offsets[i], res->offsets[i + 1] - res->offsets[i]));
                ++reads_written;
            } else if (t1 && res->cls[i] >= 2) {
                alone(t1, u1, u, names[i] + "/1"); alone(t2, u2, u, names[i] + "/2");
                ++u;
            }
        }
        mapad_merge_result_free(res);
        if (t1) { mapad_merge_result_free(t1); mapad_merge_result_free(t2); }
        if (clean) clean->back(out);
        return more;
    }
    void report(const Args& a, const char* cmd) const {
        if (a.has("merge_report")) write_merge_report(a.get("merge_report"), total, single);
        std::fprintf(stderr, "%s: %llu %s seen, %llu %s, %llu bases in, %llu bases out", cmd, (unsigned long long)total.pairs_seen, single ? "reads" : "pairs",
                     (unsigned long long)reads_written, single ? "kept" : "merged", (unsigned long long)total.bases_in, (unsigned long long)total.bases_out);
        if (!single && unmerged_single) std::fprintf(stderr, "; %llu mates of unmerged pairs go on alone, %llu dropped", (unsigned long long)singles_written, (unsigned long long)singles_dropped);
        std::fprintf(stderr, "\n");
    }
};
// FASTQ out, plain or gzip by the file's name: what `merge` and `clean` write
struct FastqWriter {
    std::string path, text;
    gzFile out;
    explicit FastqWriter(const std::string& p) : path(p) {
        const bool gz = path.size() > 3 && path.compare(path.size() - 3, 3, ".gz") == 0;
        out = gzopen(path.c_str(), gz ? "wb" : "wbT");  // "T": written as it is, no gzip
        if (!out) die("cannot write " + path);
    }
    FastqWriter(const FastqWriter&) = delete;
    ~FastqWriter() { if (out) gzclose(out); }
    void write(const std::vector<InRecord>& reads) {
        text.clear();
        for (const InRecord& r : reads) {
            text += '@'; text += r.name; text += '\n'; text += r.seq; text += "\n+\n";
            if (r.qual.size() == r.seq.size()) for (uint8_t q : r.qual) text += (char)((q == 255 ? 0 : std::min<int>(q, 93)) + 33);
            else text.append(r.seq.size(), '!');  // a record without qualities
            text += '\n';
        }
        if (!text.empty() && gzwrite(out, text.data(), (unsigned)text.size()) != (int)text.size()) die("cannot write " + path);
    }
    void close() { const int rc = gzclose(out); out = nullptr; if (rc != Z_OK) die("cannot write " + path); }
};
// `mapad-amd merge -1 R1.fastq[.gz] [-2 R2.fastq[.gz]] -o OUT.fastq[.gz] [--host] [--merge_report FILE] [the merge options of map]`; with -1 alone: single-end trimming
int cmd_merge(const Args& a, int device) {
    if (!a.has("reads1") || !a.has("output")) die("merge: -1 and -o are required");
    ReadSource in1(a.get("reads1"));
    if (in1.is_bam()) die("merge: FASTQ input only (BAM and CRAM pairs are not supported)");
    MergeStage stage(a, device, a.flag("host"), a.get("reads1"), a.get("reads2"));
    CleanStage::check_options(a, "merge");
    std::unique_ptr<CleanStage> clean_stage;
    if (CleanStage::wanted(a)) { clean_stage.reset(new CleanStage(a, device, a.flag("host"), true, "merge")); stage.clean = clean_stage.get(); }
    FastqWriter out(a.get("output"));
    const size_t chunk = (size_t)std::max<long long>(1, std::atoll(a.get("chunk_size", "250000").c_str()));
    std::vector<InRecord> reads;
    for (bool more = true; more;) {
        reads.clear();
        more = stage.next_chunk(in1, chunk, reads);
        out.write(reads);
    }
    out.close();
    stage.report(a, "merge");
    if (clean_stage) clean_stage->report(a, "merge");
    return 0;
}
// `mapad-amd clean -1 R.fastq[.gz] -o OUT.fastq[.gz] [--host] [--clean_report FILE] [the clean-up options of map]`: the clean-up alone, one pass with every op given
int cmd_clean(const Args& a, int device) {
    if (!a.has("reads1") || !a.has("output")) die("clean: -1 and -o are required");
    if (a.has("reads2")) die("clean: one file at a time (the mates of a pair are cleaned by `merge` and `map --reads2`, which keep the two files in step)");
    CleanStage::check_options(a, "clean");
    if (!CleanStage::wanted(a)) die("clean: nothing to do: give --trim_poly_g, --trim_ns, --trim_qualities or --max_dust PERMILLE");
    ReadSource in(a.get("reads1"));
    if (in.is_bam()) die("clean: FASTQ input only (BAM and CRAM are not supported)");
    CleanStage stage(a, device, a.flag("host"), false, "clean");
    FastqWriter out(a.get("output"));
    const size_t chunk = (size_t)std::max<long long>(1, std::atoll(a.get("chunk_size", "250000").c_str()));
    std::vector<InRecord> reads;
    for (bool more = true; more;) {
        reads.clear();
        more = stage.next_chunk(in, chunk, reads);
        out.write(reads);
    }
    out.close();
    stage.report(a, "clean");
    return 0;
}

// The accumulator stages as the command line sets them up and reports them: the options of `map` and of `analyse` (same names, same files), the switches of a
// context, and the report files and summary lines behind a run.  `cmd` names the subcommand in the messages.
struct StageSetup {
    std::string cmd;
    std::string damage_path, coverage_path, pileup_path, consensus_path, allele_path, dcons_path, dcons_qual_path, gt_vcf_path, gt_tsv_path, duplicates_path, dscore_hist_path,
        dscore_min, panel_path, panel_geno_path, panel_snp_path, panel_ind_path, panel_counts_path, panel_report_path, rescale_report_path;
    int damage_mode = 0, coverage_mode = 0, pileup_mode = 0, allele_mode = 0, dedup_mode = 0, dscore_mode = 0, panel_mode = 0, rescale_mode = 0;
    uint32_t pileup_min_bq = 0, pileup_mask5 = 0, pileup_mask3 = 0, consensus_min_depth = 1, consensus_min_percent = 0, allele_min_bq = 0, allele_mask5 = 0, allele_mask3 = 0,
             dcons_min_depth = 1, gt_min_depth = 1, panel_min_bq = 0, panel_mask5 = 0, panel_mask3 = 0;
    float gt_min_margin = 3.0f, gt_het_penalty = 10.0f, dcons_min_margin = 3.0f, dscore_threshold = 0.0f;
    bool genotype_on = false, rescale_keep_oq = false;
    mapad_snp_panel_rule_t panel_rule{};
    SnpPanelFile panel;

    StageSetup(const Args& a, const mapad_index_t* idx, size_t n_dev, const std::string& cmd_) : cmd(cmd_) {
        damage_path = a.get("damage_profile");
        damage_mode = damage_path.empty() ? 0 : a.flag("damage_profile_unique") ? 2 : 1;
        if (a.flag("damage_profile_unique") && damage_path.empty()) die(cmd + ": --damage_profile_unique needs --damage_profile FILE");
        coverage_path = a.get("coverage");
        coverage_mode = coverage_path.empty() ? 0 : a.flag("coverage_unique") ? 2 : 1;
        if (a.flag("coverage_unique") && coverage_path.empty()) die(cmd + ": --coverage_unique needs --coverage FILE");
        pileup_path = a.get("pileup"), consensus_path = a.get("consensus");
        pileup_mode = pileup_path.empty() && consensus_path.empty() ? 0 : a.flag("pileup_unique") ? 2 : 1;  // (--consensus alone: mode 1)
        for (const char* o : {"pileup_min_bq", "pileup_mask5", "pileup_mask3"})
            if (!a.get(o).empty() && !pileup_mode) die((cmd + ": --") + o + " needs --pileup FILE or --consensus FASTA");
        if (a.flag("pileup_unique") && !pileup_mode) die(cmd + ": --pileup_unique needs --pileup FILE or --consensus FASTA");
        for (const char* o : {"consensus_min_depth", "consensus_min_percent"})
            if (!a.get(o).empty() && !pileup_mode) die((cmd + ": --") + o + " needs --consensus FASTA or --pileup FILE");
        pileup_min_bq = (uint32_t)std::strtoul(a.get("pileup_min_bq", "0").c_str(), nullptr, 10), pileup_mask5 = (uint32_t)std::strtoul(a.get("pileup_mask5", "0").c_str(), nullptr, 10),
                       pileup_mask3 = (uint32_t)std::strtoul(a.get("pileup_mask3", "0").c_str(), nullptr, 10);
        consensus_min_depth = (uint32_t)std::strtoul(a.get("consensus_min_depth", "1").c_str(), nullptr, 10),
                       consensus_min_percent = (uint32_t)std::strtoul(a.get("consensus_min_percent", "0").c_str(), nullptr, 10);
        if (pileup_mode && (consensus_min_depth < 1 || consensus_min_percent > 100)) die(cmd + ": --consensus_min_depth is at least 1, --consensus_min_percent 0..100");
        allele_path = a.get("allele_likelihoods"), dcons_path = a.get("damage_consensus"), dcons_qual_path = a.get("damage_consensus_qual");
        gt_vcf_path = a.get("genotype_vcf"), gt_tsv_path = a.get("genotype_likelihoods");
        genotype_on = !gt_vcf_path.empty() || !gt_tsv_path.empty();
        allele_mode = allele_path.empty() && dcons_path.empty() && !genotype_on ? 0 : a.flag("allele_unique") ? 2 : 1;  // (--damage_consensus or --genotype_vcf alone: mode 1)
        for (const char* o : {"allele_min_bq", "allele_mask5", "allele_mask3"})
            if (!a.get(o).empty() && !allele_mode) die((cmd + ": --") + o + " needs --allele_likelihoods FILE, --damage_consensus FASTA or --genotype_vcf FILE");
        for (const char* o : {"damage_consensus_min_depth", "damage_consensus_min_margin"})
            if (!a.get(o).empty() && allele_path.empty() && dcons_path.empty()) die((cmd + ": --") + o + " needs --allele_likelihoods FILE or --damage_consensus FASTA");
        if (a.flag("allele_unique") && !allele_mode) die(cmd + ": --allele_unique needs --allele_likelihoods FILE, --damage_consensus FASTA or --genotype_vcf FILE");
        for (const char* o : {"genotype_min_depth", "genotype_min_margin", "genotype_het_penalty"})
            if (!a.get(o).empty() && !genotype_on) die((cmd + ": --") + o + " needs --genotype_vcf FILE or --genotype_likelihoods TSV");
        gt_min_depth = (uint32_t)std::strtoul(a.get("genotype_min_depth", "1").c_str(), nullptr, 10);
        gt_min_margin = std::strtof(a.get("genotype_min_margin", "3.0").c_str(), nullptr), gt_het_penalty = std::strtof(a.get("genotype_het_penalty", "10.0").c_str(), nullptr);
        if (genotype_on && (gt_min_depth < 1 || gt_min_margin != gt_min_margin || !(gt_het_penalty >= 0.0f)))
            die(cmd + ": --genotype_min_depth is at least 1, --genotype_min_margin a number of bits, --genotype_het_penalty a number of bits >= 0");
        if (!gt_vcf_path.empty()) {  // REF comes from the FASTA the index was built from
            FILE* f = std::fopen(a.get("reference").c_str(), "rb");
            if (!f) die(cmd + ": --genotype_vcf needs the FASTA " + a.get("reference") + " (REF bases); it cannot be read");
            std::fclose(f);
        }
        if (!dcons_qual_path.empty() && dcons_path.empty()) die(cmd + ": --damage_consensus_qual needs --damage_consensus FASTA");
        allele_min_bq = (uint32_t)std::strtoul(a.get("allele_min_bq", "0").c_str(), nullptr, 10), allele_mask5 = (uint32_t)std::strtoul(a.get("allele_mask5", "0").c_str(), nullptr, 10),
                       allele_mask3 = (uint32_t)std::strtoul(a.get("allele_mask3", "0").c_str(), nullptr, 10);
        dcons_min_depth = (uint32_t)std::strtoul(a.get("damage_consensus_min_depth", "1").c_str(), nullptr, 10);
        dcons_min_margin = std::strtof(a.get("damage_consensus_min_margin", "3.0").c_str(), nullptr);
        if (allele_mode && (dcons_min_depth < 1 || dcons_min_margin != dcons_min_margin)) die(cmd + ": --damage_consensus_min_depth is at least 1, --damage_consensus_min_margin a number of bits");
        duplicates_path = a.get("duplicates");
        dedup_mode = a.flag("exclude_duplicates") ? 2 : a.flag("mark_duplicates") ? 1 : 0;
        if (!duplicates_path.empty() && !dedup_mode) die(cmd + ": --duplicates FILE needs --mark_duplicates or --exclude_duplicates");
        // a table per device cannot see the other devices' reads: rather refused than silently under-marked
        if (dedup_mode && n_dev > 1) die(cmd + ": --mark_duplicates / --exclude_duplicates work on one device only (--devices names more than one): duplicates across devices would go unmarked");
        dscore_hist_path = a.get("damage_score_hist"), dscore_min = a.get("damage_score_min");
        dscore_mode = !dscore_min.empty() ? 2 : (a.flag("damage_score") || !dscore_hist_path.empty()) ? 1 : 0;
        dscore_threshold = 0.0f;
        if (!dscore_min.empty()) {
            char* end = nullptr;
            dscore_threshold = std::strtof(dscore_min.c_str(), &end);
            if (end == dscore_min.c_str() || *end || dscore_threshold != dscore_threshold) die(cmd + ": --damage_score_min takes a number of bits");
        }
        // SNP panel: pseudo-haploid calls at the rows of an EIGENSTRAT .snp file, counted on the GPU strand by strand
        panel_path = a.get("snp_panel"), panel_geno_path = a.get("panel_geno"), panel_snp_path = a.get("panel_snp"), panel_ind_path = a.get("panel_ind"),
                          panel_counts_path = a.get("panel_counts"), panel_report_path = a.get("panel_report");
        panel_mode = panel_path.empty() ? 0 : a.flag("panel_unique") ? 2 : 1;
        for (const char* o : {"panel_geno", "panel_snp", "panel_ind", "panel_sample", "panel_population", "panel_counts", "panel_call", "panel_min_depth", "panel_seed",
                              "panel_transitions", "panel_min_bq", "panel_mask5", "panel_mask3", "panel_report"})
            if (!a.get(o).empty() && !panel_mode) die((cmd + ": --") + o + " needs --snp_panel FILE.snp");
        if (a.flag("panel_unique") && !panel_mode) die(cmd + ": --panel_unique needs --snp_panel FILE.snp");
        if (panel_mode && panel_geno_path.empty()) die(cmd + ": --snp_panel needs --panel_geno OUT.geno");
        if ((!a.get("panel_sample").empty() || !a.get("panel_population").empty()) && panel_ind_path.empty()) die(cmd + ": --panel_sample and --panel_population need --panel_ind OUT.ind");
        const auto panel_number = [&](const char* o, const char* dflt, uint64_t max) {
            const std::string v = a.get(o, dflt);
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 20) die((cmd + ": --") + o + " takes a non-negative integer");
            errno = 0;
            const unsigned long long x = std::strtoull(v.c_str(), nullptr, 10);
            if (errno || x > max) die((cmd + ": --") + o + " is at most " + std::to_string(max));
            return (uint64_t)x;
        };
        panel_rule = mapad_snp_panel_rule_t{};
        {
            const std::string call = a.get("panel_call", "random"), tr = a.get("panel_transitions", "keep");
            if (call != "random" && call != "majority") die(cmd + ": --panel_call is random or majority");
            if (tr != "keep" && tr != "missing" && tr != "single_strand") die(cmd + ": --panel_transitions is keep, missing or single_strand");
            panel_rule.call = call == "majority"; panel_rule.transitions = tr == "keep" ? 0 : tr == "missing" ? 1 : 2;
            panel_rule.min_depth = (uint32_t)panel_number("panel_min_depth", "1", 0xFFFFFFFFull);
            panel_rule.seed = panel_number("panel_seed", "0", ~0ull);
            if (panel_mode && panel_rule.min_depth < 1) die(cmd + ": --panel_min_depth is at least 1");
        }
        panel_min_bq = (uint32_t)panel_number("panel_min_bq", "0", 255), panel_mask5 = (uint32_t)panel_number("panel_mask5", "0", 65535),
                       panel_mask3 = (uint32_t)panel_number("panel_mask3", "0", 65535);
        if (panel_mode) panel = read_snp_panel(panel_path, idx);
        rescale_report_path = a.get("rescale_report");
        rescale_keep_oq = a.flag("rescale_keep_original");
        if ((a.flag("rescale_pileup") || rescale_keep_oq || !rescale_report_path.empty()) && !a.flag("rescale_qualities"))
            die(cmd + ": --rescale_pileup, --rescale_keep_original and --rescale_report FILE need --rescale_qualities");
        if (a.flag("rescale_pileup") && !pileup_mode && !panel_mode) die(cmd + ": --rescale_pileup needs --pileup FILE or --consensus FASTA (or --snp_panel FILE.snp)");
        rescale_mode = a.flag("rescale_pileup") ? 2 : a.flag("rescale_qualities") ? 1 : 0;
    }
    // the switches of one context
    void apply(mapad_ctx_t* ctx) const {
        if (damage_mode) check(mapad_ctx_set_damage_profile(ctx, damage_mode), "mapad_ctx_set_damage_profile");
        if (coverage_mode) check(mapad_ctx_set_coverage(ctx, coverage_mode), "mapad_ctx_set_coverage");
        if (pileup_mode) check(mapad_ctx_set_pileup(ctx, pileup_mode, pileup_min_bq, pileup_mask5, pileup_mask3), "mapad_ctx_set_pileup");
        if (panel_mode)
            check(mapad_ctx_set_snp_panel(ctx, panel_mode, panel.tid.size(), panel.tid.data(), panel.pos0.data(), panel.ref.data(), panel.alt.data(), panel_min_bq, panel_mask5,
                                          panel_mask3), "mapad_ctx_set_snp_panel");
        if (allele_mode) check(mapad_ctx_set_allele_likelihoods(ctx, allele_mode, allele_min_bq, allele_mask5, allele_mask3), "mapad_ctx_set_allele_likelihoods");
        if (genotype_on) check(mapad_ctx_set_genotype_likelihoods(ctx, 1), "mapad_ctx_set_genotype_likelihoods");
        if (dedup_mode) check(mapad_ctx_set_mark_duplicates(ctx, dedup_mode), "mapad_ctx_set_mark_duplicates");
        if (dscore_mode) check(mapad_ctx_set_damage_score(ctx, dscore_mode, dscore_threshold), "mapad_ctx_set_damage_score");
        if (rescale_mode) check(mapad_ctx_set_quality_rescale(ctx, rescale_mode), "mapad_ctx_set_quality_rescale");
    }
    // the report files and the summary lines on stderr, behind the last batch; ctxs: one per device (the tables of the others are merged into the first one's)
    void report(const Args& a, const mapad_index_t* idx, const std::vector<mapad_ctx_t*>& ctxs) const {
        const size_t n_dev = ctxs.size();
        if (dedup_mode) {
            mapad_duplicates_t dup;
            check(mapad_ctx_duplicates(ctxs[0], &dup), "mapad_ctx_duplicates");
            if (!duplicates_path.empty()) {
                FILE* f = std::fopen(duplicates_path.c_str(), "w");
                if (!f) die("cannot write " + duplicates_path);
                std::fprintf(f, "#mapad-amd-duplicates v1 mode=%s bins=%d\n", dedup_mode == 2 ? "exclude" : "mark", MAPAD_DUPLICATES_BINS);
                std::fprintf(f, "#reads_seen\treads_eligible\tduplicates\tfragments\tslots\tgrows\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)dup.reads_seen, (unsigned long long)dup.reads_eligible, (unsigned long long)dup.duplicates,
                             (unsigned long long)dup.fragments, (unsigned long long)dup.slots, (unsigned long long)dup.grows, (unsigned long long)dup.batches);
                std::fprintf(f, "#members\tfragments\n");  // the library-complexity curve; the last row is >= 255
                for (int k = 1; k < MAPAD_DUPLICATES_BINS; ++k) std::fprintf(f, "%d\t%llu\n", k, (unsigned long long)dup.histogram[k]);
                if (std::fclose(f) != 0) die("cannot write " + duplicates_path);
            }
            std::fprintf(stderr, "mapad-amd: duplicates (%s): %llu of %llu mapped reads flagged (%.2f %%), %llu fragments; kernels %.3f ms over %llu batches, table of %llu slots grown %llu times\n",
                         dedup_mode == 2 ? "excluded" : "marked", (unsigned long long)dup.duplicates, (unsigned long long)dup.reads_eligible,
                         100.0 * (double)dup.duplicates / (double)std::max<uint64_t>(dup.reads_eligible, 1), (unsigned long long)dup.fragments, dup.mark_ms, (unsigned long long)dup.batches,
                         (unsigned long long)dup.slots, (unsigned long long)dup.grows);
        }
        if (dscore_mode) {  // the summary is additive: summed over the devices
            mapad_damage_scores_t sum;
            std::memset(&sum, 0, sizeof sum);
            for (size_t d = 0; d < n_dev; ++d) {
                mapad_damage_scores_t one;
                check(mapad_ctx_damage_scores(ctxs[d], &one), "mapad_ctx_damage_scores");
                sum.reads_seen += one.reads_seen; sum.reads_scored += one.reads_scored; sum.reads_below += one.reads_below; sum.informative_columns += one.informative_columns;
                sum.score_sum += one.score_sum; sum.batches += one.batches; sum.threshold_q = one.threshold_q; sum.kernel_ms += one.kernel_ms;
                for (int k = 0; k < MAPAD_DAMAGE_SCORE_BINS; ++k) sum.histogram[k] += one.histogram[k];
            }
            if (!dscore_hist_path.empty()) {
                FILE* f = std::fopen(dscore_hist_path.c_str(), "w");
                if (!f) die("cannot write " + dscore_hist_path);
                std::fprintf(f, "#mapad-amd-damage-score v1 mode=%s bins=%d threshold_q=%d\n", dscore_mode == 2 ? "filter" : "score", MAPAD_DAMAGE_SCORE_BINS, (int)sum.threshold_q);
                std::fprintf(f, "#reads_seen\treads_scored\treads_below\tinformative_columns\tscore_sum_q\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%lld\t%llu\n", (unsigned long long)sum.reads_seen, (unsigned long long)sum.reads_scored, (unsigned long long)sum.reads_below,
                             (unsigned long long)sum.informative_columns, (long long)sum.score_sum, (unsigned long long)sum.batches);
                std::fprintf(f, "#bin_start_bits\treads\n");  // half a bit per bin; the first and the last bin take everything beyond
                for (int k = 0; k < MAPAD_DAMAGE_SCORE_BINS; ++k) std::fprintf(f, "%.1f\t%llu\n", (k - 64) * 0.5, (unsigned long long)sum.histogram[k]);
                if (std::fclose(f) != 0) die("cannot write " + dscore_hist_path);
            }
            std::fprintf(stderr, "mapad-amd: damage score (%s): %llu of %llu reads scored, mean %.3f bits, %llu below %.3f bits; kernel %.3f ms over %llu batches\n",
                         dscore_mode == 2 ? "filter" : "score", (unsigned long long)sum.reads_scored, (unsigned long long)sum.reads_seen,
                         (double)sum.score_sum / 256.0 / (double)std::max<uint64_t>(sum.reads_scored, 1), (unsigned long long)sum.reads_below, (double)sum.threshold_q / 256.0, sum.kernel_ms,
                         (unsigned long long)sum.batches);
        }
        if (rescale_mode) {  // the summary is additive: summed over the devices
            mapad_rescale_t sum;
            std::memset(&sum, 0, sizeof sum);
            for (size_t d = 0; d < n_dev; ++d) {
                mapad_rescale_t one;
                check(mapad_ctx_quality_rescale(ctxs[d], &one), "mapad_ctx_quality_rescale");
                sum.reads_seen += one.reads_seen; sum.reads_rescaled += one.reads_rescaled; sum.candidate_columns[0] += one.candidate_columns[0];
                sum.candidate_columns[1] += one.candidate_columns[1]; sum.bases_changed += one.bases_changed; sum.quality_drop_sum += one.quality_drop_sum;
                sum.batches += one.batches; sum.kernel_ms += one.kernel_ms;
                for (int k = 0; k < MAPAD_RESCALE_BINS; ++k) sum.new_quality[k] += one.new_quality[k];
            }
            if (!rescale_report_path.empty()) {
                FILE* f = std::fopen(rescale_report_path.c_str(), "w");
                if (!f) die("cannot write " + rescale_report_path);
                std::fprintf(f, "#mapad-amd-rescale v1 mode=%s bins=%d\n", rescale_mode == 2 ? "pileup" : "records", MAPAD_RESCALE_BINS);
                std::fprintf(f, "#reads_seen\treads_rescaled\tcandidate_ct\tcandidate_ga\tbases_changed\tquality_drop_sum\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)sum.reads_seen, (unsigned long long)sum.reads_rescaled,
                             (unsigned long long)sum.candidate_columns[0], (unsigned long long)sum.candidate_columns[1], (unsigned long long)sum.bases_changed,
                             (unsigned long long)sum.quality_drop_sum, (unsigned long long)sum.batches);
                std::fprintf(f, "#new_quality\tbases\n");  // changed bases by their new quality; the last bin takes everything from 63 up
                for (int k = 0; k < MAPAD_RESCALE_BINS; ++k) std::fprintf(f, "%d\t%llu\n", k, (unsigned long long)sum.new_quality[k]);
                if (std::fclose(f) != 0) die("cannot write " + rescale_report_path);
            }
            std::fprintf(stderr, "mapad-amd: quality rescaling (%s): %llu of %llu reads rescaled, %llu C->T and %llu G->A columns, %llu bases changed by %.2f on average; kernel %.3f ms over %llu batches\n",
                         rescale_mode == 2 ? "pileup" : "records", (unsigned long long)sum.reads_rescaled, (unsigned long long)sum.reads_seen, (unsigned long long)sum.candidate_columns[0],
                         (unsigned long long)sum.candidate_columns[1], (unsigned long long)sum.bases_changed, (double)sum.quality_drop_sum / (double)std::max<uint64_t>(sum.bases_changed, 1),
                         sum.kernel_ms, (unsigned long long)sum.batches);
        }
        if (damage_mode) {  // the table is additive: summed over the devices
            mapad_damage_profile_t sum;
            std::memset(&sum, 0, sizeof sum);
            for (auto* c : ctxs) {
                mapad_damage_profile_t one;
                check(mapad_ctx_damage_profile(c, &one), "mapad_ctx_damage_profile");
                for (int e = 0; e < 2; ++e) for (int p = 0; p < MAPAD_DAMAGE_POSITIONS; ++p) for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) sum.counts[e][p][r][q] += one.counts[e][p][r][q];
                sum.reads += one.reads; sum.reads_seen += one.reads_seen; sum.aligned_bases += one.aligned_bases; sum.skipped_bases += one.skipped_bases;
                sum.insertions += one.insertions; sum.deletions += one.deletions; sum.batches += one.batches; sum.kernel_ms += one.kernel_ms;
            }
            auto freq = [&](int e, int p, int r, int q) {
                uint64_t den = 0;
                for (int k = 0; k < 4; ++k) den += sum.counts[e][p][r][k];
                return den ? (double)sum.counts[e][p][r][q] / (double)den : 0.0;
            };
            FILE* f = std::fopen(damage_path.c_str(), "w");
            if (!f) die("cannot write " + damage_path);
            std::fprintf(f, "#mapad-amd-damage-profile v1 mode=%s reads=%llu reads_seen=%llu positions=%d\n", damage_mode == 2 ? "unique" : "all", (unsigned long long)sum.reads,
                         (unsigned long long)sum.reads_seen, MAPAD_DAMAGE_POSITIONS);
            std::fprintf(f, "end\tpos");
            for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::fprintf(f, "\t%c>%c", "ACGT"[r], "ACGT"[q]);
            std::fprintf(f, "\tC>T_freq\tG>A_freq\n");
            for (int e = 0; e < 2; ++e)
                for (int p = 0; p < MAPAD_DAMAGE_POSITIONS; ++p) {
                    std::fprintf(f, "%s\t%d", e ? "3p" : "5p", p + 1);
                    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::fprintf(f, "\t%llu", (unsigned long long)sum.counts[e][p][r][q]);
                    std::fprintf(f, "\t%.6f\t%.6f\n", freq(e, p, 1, 3), freq(e, p, 2, 0));
                }
            if (std::fclose(f) != 0) die("cannot write " + damage_path);
            std::fprintf(stderr, "mapad-amd: damage profile (%s): %llu of %llu reads, %llu aligned bases; C>T at 5p pos 1 %.6f, G>A at 3p pos 1 %.6f; kernel %.3f ms over %llu batches\n",
                         damage_mode == 2 ? "unique" : "all", (unsigned long long)sum.reads, (unsigned long long)sum.reads_seen, (unsigned long long)sum.aligned_bases, freq(0, 0, 1, 3),
                         freq(1, 0, 2, 0), sum.kernel_ms, (unsigned long long)sum.batches);
        }
        if (coverage_mode) {  // the summary is not additive, the difference array is: the other devices' arrays into the first one's, then one finishing pass
            for (size_t d = 1; d < n_dev; ++d) check(mapad_ctx_coverage_merge(ctxs[0], ctxs[d]), "mapad_ctx_coverage_merge");
            const uint32_t nc = mapad_index_n_contigs(idx);
            std::vector<mapad_coverage_contig_t> rows(std::max<uint32_t>(nc, 1));
            mapad_coverage_t cov;
            std::memset(&cov, 0, sizeof cov);
            cov.n_contigs = nc; cov.contigs = rows.data();
            check(mapad_ctx_coverage(ctxs[0], &cov), "mapad_ctx_coverage");
            FILE* f = std::fopen(coverage_path.c_str(), "w");
            if (!f) die("cannot write " + coverage_path);
            std::fprintf(f, "#mapad-amd-coverage v1 mode=%s reads=%llu reads_seen=%llu contigs=%u bins=%d\n", coverage_mode == 2 ? "unique" : "all", (unsigned long long)cov.reads,
                         (unsigned long long)cov.reads_seen, nc, MAPAD_COVERAGE_BINS);
            std::fprintf(f, "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmaxdepth\n");
            uint64_t total = 0, covered = 0, depth_sum = 0;
            for (uint32_t t = 0; t < nc; ++t) {
                const char* name = nullptr;
                uint64_t s0 = 0, e0 = 0;
                check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                const mapad_coverage_contig_t& r = rows[t];
                std::fprintf(f, "%s\t1\t%llu\t%llu\t%llu\t%.4f\t%.6f\t%llu\n", name, (unsigned long long)r.length, (unsigned long long)r.reads, (unsigned long long)r.covered_bases,
                             100.0 * (double)r.covered_bases / (double)r.length, (double)r.depth_sum / (double)r.length, (unsigned long long)r.max_depth);
                total += r.length; covered += r.covered_bases; depth_sum += r.depth_sum;
            }
            std::fprintf(f, "#depth\tbases\n");
            for (int b = 0; b < MAPAD_COVERAGE_BINS; ++b) std::fprintf(f, "%d\t%llu\n", b, (unsigned long long)cov.hist[b]);
            if (std::fclose(f) != 0) die("cannot write " + coverage_path);
            std::fprintf(stderr, "mapad-amd: coverage (%s): %llu of %llu reads, %llu of %llu bases covered, mean depth %.6f; kernel %.3f ms over %llu batches, summary %.3f ms\n",
                         coverage_mode == 2 ? "unique" : "all", (unsigned long long)cov.reads, (unsigned long long)cov.reads_seen, (unsigned long long)covered, (unsigned long long)total,
                         (double)depth_sum / (double)std::max<uint64_t>(total, 1), cov.accumulate_ms, (unsigned long long)cov.batches, cov.summary_ms);
        }
        if (pileup_mode) {  // the calls are not additive, the counts are: the other devices' counts into the first one's, then the calls
            for (size_t d = 1; d < n_dev; ++d) check(mapad_ctx_pileup_merge(ctxs[0], ctxs[d]), "mapad_ctx_pileup_merge");
            const uint32_t nc = mapad_index_n_contigs(idx);
            std::vector<mapad_pileup_contig_t> rows(std::max<uint32_t>(nc, 1));
            mapad_pileup_t pil;
            std::memset(&pil, 0, sizeof pil);
            pil.n_contigs = nc; pil.contigs = rows.data();
            check(mapad_ctx_pileup(ctxs[0], consensus_min_depth, consensus_min_percent, &pil), "mapad_ctx_pileup");
            uint64_t total = 0, covered = 0, called = 0;
            for (uint32_t t = 0; t < nc; ++t) { total += rows[t].length; covered += rows[t].sites_covered; called += rows[t].sites_called; }
            if (!pileup_path.empty()) {
                FILE* f = std::fopen(pileup_path.c_str(), "w");
                if (!f) die("cannot write " + pileup_path);
                std::fprintf(f, "#mapad-amd-pileup v1 mode=%s min_bq=%u mask5=%u mask3=%u min_depth=%u min_percent=%u contigs=%u\n", pileup_mode == 2 ? "unique" : "all", pil.min_base_quality,
                             pil.mask5, pil.mask3, pil.min_depth, pil.min_percent, nc);
                std::fprintf(f, "#reads\treads_seen\tcolumns_counted\tcolumns_not_acgt\tcolumns_masked\tcolumns_low_quality\tdeleted_columns\tinsertions\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)pil.reads, (unsigned long long)pil.reads_seen, (unsigned long long)pil.columns_counted,
                             (unsigned long long)pil.columns_not_acgt, (unsigned long long)pil.columns_masked, (unsigned long long)pil.columns_low_quality,
                             (unsigned long long)pil.deleted_columns, (unsigned long long)pil.insertions, (unsigned long long)pil.batches);
                std::fprintf(f, "#rname\tlength\tsites_covered\tsites_deep\tsites_called\tcalled_A\tcalled_C\tcalled_G\tcalled_T\tsum_A\tsum_C\tsum_G\tsum_T\tmaxdepth\n");
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    const mapad_pileup_contig_t& r = rows[t];
                    std::fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu", name, (unsigned long long)r.length, (unsigned long long)r.sites_covered, (unsigned long long)r.sites_deep, (unsigned long long)r.sites_called);
                    for (int b = 0; b < 4; ++b) std::fprintf(f, "\t%llu", (unsigned long long)r.called[b]);
                    for (int b = 0; b < 4; ++b) std::fprintf(f, "\t%llu", (unsigned long long)r.base_sum[b]);
                    std::fprintf(f, "\t%llu\n", (unsigned long long)r.max_depth);
                }
                if (std::fclose(f) != 0) die("cannot write " + pileup_path);
            }
            if (!consensus_path.empty()) {  // one record per contig, 60 columns, the index's names
                FILE* f = std::fopen(consensus_path.c_str(), "w");
                if (!f) die("cannot write " + consensus_path);
                constexpr uint64_t kPiece = 60ull << 16;  // positions per call: whole lines
                std::vector<uint8_t> piece;
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    std::fprintf(f, ">%s\n", name);
                    for (uint64_t at = 0; at < rows[t].length; at += kPiece) {
                        const uint64_t len = std::min<uint64_t>(kPiece, rows[t].length - at);
                        piece.resize(len);
                        check(mapad_ctx_pileup_consensus(ctxs[0], t, at, len, consensus_min_depth, consensus_min_percent, piece.data()), "mapad_ctx_pileup_consensus");
                        for (uint64_t i = 0; i < len; i += 60) {
                            std::fwrite(piece.data() + i, 1, (size_t)std::min<uint64_t>(60, len - i), f);
                            std::fputc('\n', f);
                        }
                    }
                }
                if (std::fclose(f) != 0) die("cannot write " + consensus_path);
            }
            std::fprintf(stderr, "mapad-amd: pileup (%s): %llu of %llu reads, %llu columns counted, %llu of %llu bases covered, %llu called (min depth %u, min percent %u); kernel %.3f ms over %llu batches, summary %.3f ms\n",
                         pileup_mode == 2 ? "unique" : "all", (unsigned long long)pil.reads, (unsigned long long)pil.reads_seen, (unsigned long long)pil.columns_counted, (unsigned long long)covered,
                         (unsigned long long)total, (unsigned long long)called, pil.min_depth, pil.min_percent, pil.accumulate_ms, (unsigned long long)pil.batches, pil.summary_ms);
        }
        if (panel_mode) {  // the calls are not additive, the counts are: the other devices' counts into the first one's, then the calls
            for (size_t d = 1; d < n_dev; ++d) check(mapad_ctx_snp_panel_merge(ctxs[0], ctxs[d]), "mapad_ctx_snp_panel_merge");
            const uint64_t n_rows = panel.tid.size();
            mapad_snp_panel_t pan;
            check(mapad_ctx_snp_panel(ctxs[0], &panel_rule, &pan), "mapad_ctx_snp_panel");
            std::vector<uint8_t> calls(n_rows);
            check(mapad_ctx_snp_panel_calls(ctxs[0], 0, n_rows, &panel_rule, calls.data()), "mapad_ctx_snp_panel_calls");
            const char* call_name = panel_rule.call ? "majority" : "random";
            const char* tr_name = panel_rule.transitions == 0 ? "keep" : panel_rule.transitions == 1 ? "missing" : "single_strand";
            write_lines(panel_geno_path, [&](FILE* f) { for (uint64_t i = 0; i < n_rows; ++i) std::fprintf(f, "%c\n", (char)calls[i]); });  // one sample: one character per line
            if (!panel_snp_path.empty()) write_lines(panel_snp_path, [&](FILE* f) { for (const auto& ln : panel.lines) std::fprintf(f, "%s\n", ln.c_str()); });
            if (!panel_ind_path.empty())
                write_lines(panel_ind_path, [&](FILE* f) { std::fprintf(f, "%s\tU\t%s\n", a.get("panel_sample", "sample").c_str(), a.get("panel_population", "Unknown").c_str()); });
            if (!panel_counts_path.empty()) {
                std::vector<uint32_t> cells(n_rows * 8);
                check(mapad_ctx_snp_panel_counts(ctxs[0], 0, n_rows, cells.data()), "mapad_ctx_snp_panel_counts");
                write_lines(panel_counts_path, [&](FILE* f) {
                    std::fprintf(f, "#mapad-amd-snp-panel v1 mode=%s min_bq=%u mask5=%u mask3=%u call=%s min_depth=%u transitions=%s seed=%llu\n", panel_mode == 2 ? "unique" : "all",
                                 pan.min_base_quality, pan.mask5, pan.mask3, call_name, panel_rule.min_depth, tr_name, (unsigned long long)panel_rule.seed);
                    std::fprintf(f, "#id\tchrom\tpos\tref\talt\tfwd_A\tfwd_C\tfwd_G\tfwd_T\trev_A\trev_C\trev_G\trev_T\tcall\n");
                    for (uint64_t i = 0; i < n_rows; ++i) {
                        std::fprintf(f, "%s\t%s\t%llu\t%c\t%c", panel.id[i].c_str(), panel.chrom[i].c_str(), (unsigned long long)panel.physpos[i], (char)panel.ref[i], (char)panel.alt[i]);
                        for (uint32_t k = 0; k < 8; ++k) std::fprintf(f, "\t%u", cells[i * 8 + k]);
                        std::fprintf(f, "\t%c\n", (char)calls[i]);
                    }
                });
            }
            if (!panel_report_path.empty())
                write_lines(panel_report_path, [&](FILE* f) {
                    std::fprintf(f, "mode\t%s\nmin_bq\t%u\nmask5\t%u\nmask3\t%u\ncall\t%s\nmin_depth\t%u\ntransitions\t%s\nseed\t%llu\n", panel_mode == 2 ? "unique" : "all",
                                 pan.min_base_quality, pan.mask5, pan.mask3, call_name, panel_rule.min_depth, tr_name, (unsigned long long)panel_rule.seed);
                    const std::pair<const char*, uint64_t> words[] = {
                        {"n_rows", pan.n_rows}, {"n_slots", pan.n_slots}, {"reads_seen", pan.reads_seen}, {"reads", pan.reads}, {"reads_on_panel", pan.reads_on_panel},
                        {"columns_counted", pan.columns_counted}, {"columns_not_acgt", pan.columns_not_acgt}, {"columns_masked", pan.columns_masked},
                        {"columns_low_quality", pan.columns_low_quality}, {"columns_deleted", pan.columns_deleted}, {"rows", pan.rows}, {"rows_unplaced", pan.rows_unplaced},
                        {"rows_bad_alleles", pan.rows_bad_alleles}, {"rows_transition", pan.rows_transition}, {"rows_covered", pan.rows_covered}, {"rows_called", pan.rows_called},
                        {"called_ref", pan.called_ref}, {"called_alt", pan.called_alt}, {"transitions_called", pan.transitions_called}, {"obs_ref", pan.obs_ref},
                        {"obs_alt", pan.obs_alt}, {"obs_other", pan.obs_other}, {"max_depth", pan.max_depth}, {"batches", pan.batches}};
                    for (const auto& w : words) std::fprintf(f, "%s\t%llu\n", w.first, (unsigned long long)w.second);
                });
            std::fprintf(stderr, "mapad-amd: snp panel (%s): %llu of %llu reads, %llu on the panel, %llu columns counted; %llu of %llu rows called (%s, min depth %u, transitions %s): %llu ref, %llu alt; kernel %.3f ms over %llu batches, summary %.3f ms\n",
                         panel_mode == 2 ? "unique" : "all", (unsigned long long)pan.reads, (unsigned long long)pan.reads_seen, (unsigned long long)pan.reads_on_panel,
                         (unsigned long long)pan.columns_counted, (unsigned long long)pan.rows_called, (unsigned long long)pan.rows, call_name, panel_rule.min_depth, tr_name,
                         (unsigned long long)pan.called_ref, (unsigned long long)pan.called_alt, pan.accumulate_ms, (unsigned long long)pan.batches, pan.summary_ms);
        }
        if (allele_mode) {  // the calls are not additive, the sums are: the other devices' cells into the first one's, then the calls
            for (size_t d = 1; d < n_dev; ++d) {
                check(mapad_ctx_allele_merge(ctxs[0], ctxs[d]), "mapad_ctx_allele_merge");
                if (genotype_on) check(mapad_ctx_genotype_merge(ctxs[0], ctxs[d]), "mapad_ctx_genotype_merge");
            }
        }
        if (allele_mode && (!allele_path.empty() || !dcons_path.empty())) {
            const uint32_t nc = mapad_index_n_contigs(idx);
            std::vector<mapad_allele_contig_t> rows(std::max<uint32_t>(nc, 1));
            mapad_allele_t al;
            std::memset(&al, 0, sizeof al);
            al.n_contigs = nc; al.contigs = rows.data();
            check(mapad_ctx_allele_summary(ctxs[0], dcons_min_depth, dcons_min_margin, &al), "mapad_ctx_allele_summary");
            uint64_t total = 0, covered = 0, called = 0;
            for (uint32_t t = 0; t < nc; ++t) { total += rows[t].length; covered += rows[t].sites_covered; called += rows[t].sites_called; }
            if (!allele_path.empty()) {
                FILE* f = std::fopen(allele_path.c_str(), "w");
                if (!f) die("cannot write " + allele_path);
                std::fprintf(f, "#mapad-amd-allele-likelihoods v1 mode=%s min_bq=%u mask5=%u mask3=%u min_depth=%u min_margin_q=%d contigs=%u\n", allele_mode == 2 ? "unique" : "all",
                             al.min_base_quality, al.mask5, al.mask3, al.min_depth, al.min_margin_q, nc);
                std::fprintf(f, "#reads\treads_seen\tcolumns_counted\tcolumns_not_acgt\tcolumns_masked\tcolumns_low_quality\tdeleted_columns\tinsertions\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)al.reads, (unsigned long long)al.reads_seen, (unsigned long long)al.columns_counted,
                             (unsigned long long)al.columns_not_acgt, (unsigned long long)al.columns_masked, (unsigned long long)al.columns_low_quality,
                             (unsigned long long)al.deleted_columns, (unsigned long long)al.insertions, (unsigned long long)al.batches);
                std::fprintf(f, "#rname\tlength\tsites_covered\tsites_deep\tsites_called\tcalled_A\tcalled_C\tcalled_G\tcalled_T\tmaxdepth\tmargin_sum_q\n");
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    const mapad_allele_contig_t& r = rows[t];
                    std::fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu", name, (unsigned long long)r.length, (unsigned long long)r.sites_covered, (unsigned long long)r.sites_deep, (unsigned long long)r.sites_called);
                    for (int b = 0; b < 4; ++b) std::fprintf(f, "\t%llu", (unsigned long long)r.called[b]);
                    std::fprintf(f, "\t%llu\t%llu\n", (unsigned long long)r.max_depth, (unsigned long long)r.margin_sum_q);
                }
                if (std::fclose(f) != 0) die("cannot write " + allele_path);
            }
            if (!dcons_path.empty()) {  // one record per contig, 60 columns, the index's names; the qualities one line per contig
                FILE* f = std::fopen(dcons_path.c_str(), "w");
                if (!f) die("cannot write " + dcons_path);
                FILE* fq = dcons_qual_path.empty() ? nullptr : std::fopen(dcons_qual_path.c_str(), "w");
                if (!dcons_qual_path.empty() && !fq) die("cannot write " + dcons_qual_path);
                constexpr uint64_t kPiece = 60ull << 16;  // positions per call: whole lines
                std::vector<uint8_t> piece, qual;
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    std::fprintf(f, ">%s\n", name);
                    for (uint64_t at = 0; at < rows[t].length; at += kPiece) {
                        const uint64_t len = std::min<uint64_t>(kPiece, rows[t].length - at);
                        piece.resize(len); qual.resize(len);
                        check(mapad_ctx_allele_consensus(ctxs[0], t, at, len, dcons_min_depth, dcons_min_margin, piece.data(), qual.data()), "mapad_ctx_allele_consensus");
                        for (uint64_t i = 0; i < len; i += 60) {
                            std::fwrite(piece.data() + i, 1, (size_t)std::min<uint64_t>(60, len - i), f);
                            std::fputc('\n', f);
                        }
                        if (fq) {
                            for (uint64_t i = 0; i < len; ++i) qual[i] = (uint8_t)(33 + std::min<uint32_t>(qual[i], 93));
                            std::fwrite(qual.data(), 1, (size_t)len, fq);
                        }
                    }
                    if (fq) std::fputc('\n', fq);
                }
                if (std::fclose(f) != 0) die("cannot write " + dcons_path);
                if (fq && std::fclose(fq) != 0) die("cannot write " + dcons_qual_path);
            }
            std::fprintf(stderr, "mapad-amd: allele likelihoods (%s): %llu of %llu reads, %llu columns counted, %llu of %llu bases covered, %llu called (min depth %u, min margin %.3f bits); kernel %.3f ms over %llu batches, summary %.3f ms\n",
                         allele_mode == 2 ? "unique" : "all", (unsigned long long)al.reads, (unsigned long long)al.reads_seen, (unsigned long long)al.columns_counted, (unsigned long long)covered,
                         (unsigned long long)total, (unsigned long long)called, al.min_depth, (double)al.min_margin_q / 256.0, al.accumulate_ms, (unsigned long long)al.batches, al.summary_ms);
        }
        if (genotype_on) {
            const uint32_t nc = mapad_index_n_contigs(idx);
            std::vector<mapad_genotype_contig_t> rows(std::max<uint32_t>(nc, 1));
            mapad_genotype_t gs;
            std::memset(&gs, 0, sizeof gs);
            gs.n_contigs = nc; gs.contigs = rows.data();
            check(mapad_ctx_genotype_summary(ctxs[0], gt_min_depth, gt_min_margin, gt_het_penalty, &gs), "mapad_ctx_genotype_summary");
            std::vector<mapad_allele_contig_t> arows(std::max<uint32_t>(nc, 1));
            mapad_allele_t al;  // the scalars are the allele accumulator's: the same reads and columns
            std::memset(&al, 0, sizeof al);
            al.n_contigs = nc; al.contigs = arows.data();
            check(mapad_ctx_allele_summary(ctxs[0], gt_min_depth, gt_min_margin, &al), "mapad_ctx_allele_summary");
            static const char* const GT_NAME[10] = {"AA", "CC", "GG", "TT", "AC", "AG", "AT", "CG", "CT", "GT"};
            uint64_t total = 0, covered = 0, called = 0, het = 0;
            for (uint32_t t = 0; t < nc; ++t) { total += rows[t].length; covered += rows[t].sites_covered; called += rows[t].sites_called; for (int g = 4; g < 10; ++g) het += rows[t].called[g]; }
            if (!gt_tsv_path.empty()) {
                FILE* f = std::fopen(gt_tsv_path.c_str(), "w");
                if (!f) die("cannot write " + gt_tsv_path);
                std::fprintf(f, "#mapad-amd-genotype-likelihoods v1 mode=%s min_bq=%u mask5=%u mask3=%u min_depth=%u min_margin_q=%d het_penalty_q=%d contigs=%u\n", allele_mode == 2 ? "unique" : "all",
                             al.min_base_quality, al.mask5, al.mask3, gs.min_depth, gs.min_margin_q, gs.het_penalty_q, nc);
                std::fprintf(f, "#reads\treads_seen\tcolumns_counted\tcolumns_not_acgt\tcolumns_masked\tcolumns_low_quality\tdeleted_columns\tinsertions\tbatches\n");
                std::fprintf(f, "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)al.reads, (unsigned long long)al.reads_seen, (unsigned long long)al.columns_counted,
                             (unsigned long long)al.columns_not_acgt, (unsigned long long)al.columns_masked, (unsigned long long)al.columns_low_quality,
                             (unsigned long long)al.deleted_columns, (unsigned long long)al.insertions, (unsigned long long)gs.batches);
                std::fprintf(f, "#rname\tlength\tsites_covered\tsites_deep\tsites_called");
                for (int g = 0; g < 10; ++g) std::fprintf(f, "\tcalled_%s", GT_NAME[g]);
                std::fprintf(f, "\tmaxdepth\tmargin_sum_q\n");
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    const mapad_genotype_contig_t& r = rows[t];
                    std::fprintf(f, "%s\t%llu\t%llu\t%llu\t%llu", name, (unsigned long long)r.length, (unsigned long long)r.sites_covered, (unsigned long long)r.sites_deep, (unsigned long long)r.sites_called);
                    for (int g = 0; g < 10; ++g) std::fprintf(f, "\t%llu", (unsigned long long)r.called[g]);
                    std::fprintf(f, "\t%llu\t%llu\n", (unsigned long long)r.max_depth, (unsigned long long)r.margin_sum_q);
                }
                if (std::fclose(f) != 0) die("cannot write " + gt_tsv_path);
            }
            uint64_t n_records = 0;
            if (!gt_vcf_path.empty()) {  // VCF 4.2, piece by piece: calls, het cells, allele cells and depths of one window at a time
                std::vector<std::string> fa_names;
                std::vector<std::vector<uint8_t>> fa_seqs;
                read_fasta(a.get("reference"), fa_names, fa_seqs);  // (the whole FASTA in host memory, a byte per base — not the cells, which come piece by piece)
                if (fa_seqs.size() != nc) die(cmd + ": --genotype_vcf: the FASTA " + a.get("reference") + " does not have the index's contigs");
                FILE* f = std::fopen(gt_vcf_path.c_str(), "w");
                if (!f) die("cannot write " + gt_vcf_path);
                std::fprintf(f, "##fileformat=VCFv4.2\n##source=mapad-amd %s\n##reference=%s\n", mapad_version(), a.get("reference").c_str());
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    if (fa_names[t] != name || fa_seqs[t].size() != rows[t].length)
                        die(cmd + ": --genotype_vcf: contig " + std::to_string(t + 1) + " of the FASTA " + a.get("reference") + " (" + fa_names[t] + ") is not the index's (" + name + ") by name or by length");
                    std::fprintf(f, "##contig=<ID=%s,length=%llu>\n", name, (unsigned long long)rows[t].length);
                }
                std::fprintf(f, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Alignment columns counted at the site\">\n"
                                "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the margin over the second-best genotype, phred-scaled, at most 99\">\n"
                                "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods (het penalty included) relative to the best, at most 255\">\n"
                                "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n");
                const int32_t pq = gs.het_penalty_q;
                constexpr uint64_t kPiece = 1ull << 20;
                std::vector<uint8_t> gt, gq;
                std::vector<int32_t> hetc, ll;
                std::vector<uint32_t> depth;
                for (uint32_t t = 0; t < nc; ++t) {
                    const char* name = nullptr;
                    uint64_t s0 = 0, e0 = 0;
                    check(mapad_index_contig(idx, t, &name, &s0, &e0), "mapad_index_contig");
                    for (uint64_t at = 0; at < rows[t].length; at += kPiece) {
                        const uint64_t len = std::min<uint64_t>(kPiece, rows[t].length - at);
                        gt.resize(len); gq.resize(len); hetc.resize(len * 6); ll.resize(len * 4); depth.resize(len);
                        check(mapad_ctx_genotype_calls(ctxs[0], t, at, len, gt_min_depth, gt_min_margin, gt_het_penalty, gt.data(), gq.data()), "mapad_ctx_genotype_calls");
                        check(mapad_ctx_genotype_cells(ctxs[0], t, at, len, hetc.data()), "mapad_ctx_genotype_cells");
                        check(mapad_ctx_allele_cells(ctxs[0], t, at, len, ll.data(), depth.data()), "mapad_ctx_allele_cells");
                        for (uint64_t i = 0; i < len; ++i) {
                            if (gt[i] > 9) continue;  // no call
                            const char refc = (char)std::toupper((int)fa_seqs[t][at + i]);
                            const uint32_t ref = refc == 'A' ? 0u : refc == 'C' ? 1u : refc == 'G' ? 2u : refc == 'T' ? 3u : 4u;
                            if (ref > 3 || gt[i] == ref) continue;  // REF not A/C/G/T: skipped; homozygous for the reference base: no record
                            const uint32_t x = mapad::genotype_allele(gt[i], 0), y = mapad::genotype_allele(gt[i], 1);
                            uint32_t alleles[3] = {ref, 0, 0}, n_all = 1;  // REF, then the called non-reference alleles in A < C < G < T order
                            if (x != ref) alleles[n_all++] = x;
                            if (y != ref && y != x) alleles[n_all++] = y;
                            auto vcf_index = [&](uint32_t b) -> uint32_t { for (uint32_t k = 0; k < n_all; ++k) if (alleles[k] == b) return k; return 0; };
                            uint32_t i1 = vcf_index(x), i2 = vcf_index(y);
                            if (i1 > i2) std::swap(i1, i2);
                            int64_t g[mapad::GT_COUNT], best = 0, margin_q = 0;  // the ten values and the best of them, by the rule the device called with
                            if (mapad::genotype_call(ll.data() + i * 4, hetc.data() + i * 6, depth[i], gt_min_depth, gs.min_margin_q, pq, g, best, margin_q) != gt[i])
                                die(cmd + ": --genotype_vcf: the cells of " + std::string(name) + ":" + std::to_string(at + i + 1) + " do not give the device's call");
                            std::fprintf(f, "%s\t%llu\t.\t%c\t", name, (unsigned long long)(at + i + 1), refc);
                            for (uint32_t k = 1; k < n_all; ++k) std::fprintf(f, "%s%c", k > 1 ? "," : "", "ACGT"[alleles[k]]);
                            std::fprintf(f, "\t.\t.\t.\tGT:DP:GQ:PL\t%u/%u:%u:%u:", i1, i2, depth[i], (unsigned)gq[i]);
                            bool first = true;  // the VCF's genotype order: for b = 0..n-1, for a = 0..b: (a, b)
                            for (uint32_t b = 0; b < n_all; ++b)
                                for (uint32_t a2 = 0; a2 <= b; ++a2) {
                                    const uint32_t lo = std::min(alleles[a2], alleles[b]), hi = std::max(alleles[a2], alleles[b]);
                                    std::fprintf(f, "%s%u", first ? "" : ",", mapad::genotype_pl(best, g[lo == hi ? lo : mapad::genotype_of_pair(lo, hi)]));
                                    first = false;
                                }
                            std::fputc('\n', f);
                            n_records += 1;
                        }
                    }
                }
                if (std::fclose(f) != 0) die("cannot write " + gt_vcf_path);
            }
            std::fprintf(stderr, "mapad-amd: genotype likelihoods (%s): %llu of %llu reads, %llu columns counted, %llu of %llu bases covered, %llu called, %llu heterozygous, %llu VCF records (min depth %u, min margin %.3f bits, het penalty %.3f bits); kernel %.3f ms over %llu batches, summary %.3f ms\n",
                         allele_mode == 2 ? "unique" : "all", (unsigned long long)al.reads, (unsigned long long)al.reads_seen, (unsigned long long)al.columns_counted, (unsigned long long)covered,
                         (unsigned long long)total, (unsigned long long)called, (unsigned long long)het, (unsigned long long)n_records, gs.min_depth, (double)gs.min_margin_q / 256.0,
                         (double)gs.het_penalty_q / 256.0, gs.accumulate_ms, (unsigned long long)gs.batches, gs.summary_ms);
        }
    }
};

int cmd_map(const Args& a, uint64_t seed, const std::vector<int>& devices, const std::string& cmdline) {
    for (const char* req : {"reads", "reference", "output", "library", "five_prime_overhang", "ds_deamination_rate", "ss_deamination_rate", "indel_rate"})
        if (!a.has(req)) die(std::string("map: --") + req + " is required");
    if (!a.has("poisson_prob") && !a.has("as_cutoff")) die("map: either -p or -c is required");
    const std::string lib = a.get("library");
    if (lib != "single_stranded" && lib != "double_stranded") die("map: --library must be single_stranded or double_stranded");
    if (lib == "single_stranded" && !a.has("three_prime_overhang")) die("map: -t is required for single_stranded libraries");
    mapad_params_t prm;
    check(mapad_params_from_cli(&prm, lib == "single_stranded" ? MAPAD_LIBRARY_SINGLE_STRANDED : MAPAD_LIBRARY_DOUBLE_STRANDED, a.f("five_prime_overhang", 0),
                                a.f("three_prime_overhang", 0), a.f("ds_deamination_rate", 0), a.f("ss_deamination_rate", 0), a.f("divergence", 0.02f),
                                a.has("poisson_prob") ? a.f("poisson_prob", 0) : -1.0f, a.f("as_cutoff", 0), a.f("as_cutoff_exponent", 1.0f), a.f("indel_rate", 0),
                                a.f("gap_extension_penalty", 1.0f), std::atoi(a.get("gap_dist_ends", "5").c_str()), std::atoi(a.get("max_num_gaps_open", "2").c_str()),
                                a.flag("ignore_base_quality"), a.flag("no_search_limit_recovery"), std::strtoull(a.get("chunk_size", "250000").c_str(), nullptr, 10)),
          "mapad_params_from_cli");
    const auto t_start = std::chrono::steady_clock::now();
    mapad_index_t* idx = nullptr;
    check(mapad_index_open(a.get("reference").c_str(), &idx), "mapad_index_open");
    // chunks in flight per device: the serial tail of a chunk (its few heaviest reads) runs beside the bulk of the following ones.  On a text of >= 2^31
    // rows a read costs three times the pops and a chunk's tail is longer: 8 in flight map 8 % more reads/s than 4 there (3 Gbp, 8 M reads; 16 are slower again)
    // Launches per chunk.  On a text of >= 2^31 rows a read costs three times the pops, and a launch is not over before its heaviest read is (a serial chain of up to
    // ~0.5 s at 50 bp) while its bulk needs a tenth of that: every launch leaves wavefronts behind that idle on their last reads.  There --coalesce 4 (the default)
    // hands the device four chunks of --batch_size reads as ONE launch; the records do not depend on it (one seed per read of the run, below), only the XD tag's
    // granularity does (chunk wall time / reads, mapping.rs:912-918).
    const bool big_text = mapad_index_text_len(idx) >= (1ull << 31);
    const uint64_t coalesce = std::max<uint64_t>(1, std::min<uint64_t>(std::strtoull(a.get("coalesce", big_text ? "4" : "1").c_str(), nullptr, 10), 64));
    // --coalesce_steady N (round 6): launches behind the first `in_flight` ones take N chunks.  Bigger launches from the start map faster once the pipeline is full (3 Gbp,
    // same box, profiles/r06/cli_sweep_c4.txt: 3.03 M reads/s behind the first chunk with 1 M-read launches, 3.25 M with 2.5 M, 3.59 M with 5 M) but fill it slower
    // (2.1 / 5.3 / 8.2 s until the first chunk is on disk).  Starting small and growing was measured and is NOT the default: on the same 24 M reads the run that goes on
    // with 2 M-read launches is slower throughout (2.65 M reads/s behind the first chunk against 2.97 M, 11.0 s against 9.9 s; profiles/r06/cli_sweep_ramp_c4.txt) —
    // four 2 M-read batches in flight on top of the first four leave the device worker waiting longer per fetch than they save per launch.
    const uint64_t coalesce_steady = std::max<uint64_t>(coalesce, std::min<uint64_t>(std::strtoull(a.get("coalesce_steady", "0").c_str(), nullptr, 10), 64));
    const uint64_t chunk_reads_first = prm.chunk_size * coalesce, chunk_reads_max = prm.chunk_size * coalesce_steady;
    const char* in_flight_default = "4";
    const int in_flight = std::max(1, std::min(std::atoi(a.get("in_flight", in_flight_default).c_str()), 16));
    const size_t n_dev = devices.size();
    const bool collapse_duplicates = a.flag("collapse_duplicates");
    std::atomic<uint64_t> n_collapse_reads{0}, n_collapse_groups{0};  // per slice: reads / distinct reads (mapad_last_collapse_info)
    const StageSetup st(a, idx, n_dev, "map");
    const int dedup_mode = st.dedup_mode, dscore_mode = st.dscore_mode, rescale_mode = st.rescale_mode;
    const bool rescale_keep_oq = st.rescale_keep_oq;
    std::vector<mapad_ctx_t*> ctxs(n_dev, nullptr);
    for (size_t d = 0; d < n_dev; ++d) {  // the read-only index is replicated into every GPU's HBM
        check(mapad_ctx_create(idx, &prm, devices[d], &ctxs[d]), "mapad_ctx_create");
        check(mapad_ctx_set_fetch_d_arrays(ctxs[d], 0), "mapad_ctx_set_fetch_d_arrays");
        if (collapse_duplicates) check(mapad_ctx_set_collapse_duplicates(ctxs[d], 1), "mapad_ctx_set_collapse_duplicates");
        st.apply(ctxs[d]);
        check(mapad_ctx_set_pipeline_depth(ctxs[d], in_flight), "mapad_ctx_set_pipeline_depth");
        const uint64_t per_dev = (chunk_reads_max + n_dev - 1) / n_dev;  // both batch slots' buffers up front (typical short reads; longer ones grow them)
        check(mapad_ctx_reserve(ctxs[d], per_dev, per_dev * 64, 128, 1), "mapad_ctx_reserve");
    }
    const double t_load = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    ReadSource src(a.get("reads"));
    // --reads2 / --trim_adapter: the reader merges the pairs (trims the reads) of a chunk on the first device before anything else sees them
    std::unique_ptr<MergeStage> merge_stage;
    if (a.has("reads2") && a.flag("trim_adapter")) die("map: --trim_adapter is the single-end mode; with --reads2 the adapters of both mates are trimmed anyway");
    if (a.has("unmerged") && !a.has("reads2")) die("map: --unmerged says what becomes of pairs that do not merge and needs --reads2");
    if (!a.has("reads2") && !a.flag("trim_adapter"))
        for (const char* k : {"adapter1", "adapter2", "merge_min_overlap", "trim_min_overlap", "merge_max_mismatch_permille", "merge_min_length", "merge_max_quality", "merge_report"})
            if (a.has(k)) die(std::string("map: --") + k + " does nothing without --reads2 or --trim_adapter (no adapter is trimmed, no pair merged)");
    if (a.has("reads2") || a.flag("trim_adapter")) {
        if (src.is_bam()) die("map: --reads2 and --trim_adapter take FASTQ input only (BAM and CRAM are not supported)");
        merge_stage.reset(new MergeStage(a, devices[0], false, a.get("reads"), a.get("reads2")));
    }
    // --trim_poly_g / --trim_ns / --trim_qualities / --max_dust: the clean-up, around the merge stage or, without one, alone in the reader
    CleanStage::check_options(a, "map");
    std::unique_ptr<CleanStage> clean_stage;
    if (CleanStage::wanted(a)) {
        if (src.is_bam()) die("map: --trim_poly_g, --trim_ns, --trim_qualities and --max_dust take FASTQ input only (BAM and CRAM are not supported)");
        clean_stage.reset(new CleanStage(a, devices[0], false, merge_stage != nullptr, "map"));
        if (merge_stage) merge_stage->clean = clean_stage.get();
    }
    const std::string rg = a.get("read_group");
    BgzfWriter out(a.get("output"), a.flag("force_overwrite"));
    {   // BAM header
        const std::string text = make_header(src.header_text(), idx, rg, cmdline);
        std::vector<uint8_t> h = {'B', 'A', 'M', 1};
        const uint32_t l_text = (uint32_t)text.size(), n_ref = mapad_index_n_contigs(idx);
        h.insert(h.end(), (const uint8_t*)&l_text, (const uint8_t*)&l_text + 4);
        h.insert(h.end(), text.begin(), text.end());
        h.insert(h.end(), (const uint8_t*)&n_ref, (const uint8_t*)&n_ref + 4);
        for (uint32_t i = 0; i < n_ref; ++i) {
            const char* name; uint64_t s, e;
            check(mapad_index_contig(idx, i, &name, &s, &e), "mapad_index_contig");
            const uint32_t l_name = (uint32_t)std::strlen(name) + 1, l_ref = (uint32_t)(e - s + 1);
            h.insert(h.end(), (const uint8_t*)&l_name, (const uint8_t*)&l_name + 4);
            h.insert(h.end(), name, name + l_name);
            h.insert(h.end(), (const uint8_t*)&l_ref, (const uint8_t*)&l_ref + 4);
        }
        out.write(h.data(), h.size());
    }
    // Reader and writer fan every chunk out to short-lived bursts of up to 32 threads (parsing; BAM encoding + BGZF deflate) and do the rest of a chunk themselves.
    // Round 5 replaced this by standing pools sized to the cgroup's CPU share (a source thread, a parse pool with ordered emit, an encode pool working on pieces of a
    // chunk, an ordered writer: reader 1.5 s and writer 0.1 s busy instead of 5.5 s each) — and measured it 15-25 % SLOWER end to end on the same box with the same
    // library (24 M reads at C4: 11.4-13.3 s against 9.7-9.8 s; profiles/r05/cli_sweep_c4.txt): the bursts finish a chunk's host work in a fifth of a second and leave
    // the CPUs to the device worker in between, the pools keep 10 threads busy all the time.  The pools are in the history (commit d19f153), not in the tree.
    const unsigned host_threads = std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
    std::vector<std::unique_ptr<BoundedQueue<ChunkPtr>>> dev_q;
    for (size_t d = 0; d < n_dev; ++d) dev_q.emplace_back(new BoundedQueue<ChunkPtr>(2));  // read ahead; `in_flight` more are on the device
    BoundedQueue<ChunkPtr> rec_q(4), done_q(4);
    std::atomic<bool> failed{false};
    std::atomic<uint64_t> us_reader{0}, us_device{0}, us_writer{0}, us_submit{0}, us_fetch{0}, us_records{0}, us_text{0};  // busy time of the three stages (the slowest one sets the throughput)
    auto now_us = [] { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    std::string fail_msg;
    std::mutex fail_mu;
    auto fail = [&](const std::string& m) { std::lock_guard<std::mutex> l(fail_mu); if (!failed.exchange(true)) fail_msg = m; };

    // ---- reader ----
    std::thread reader([&] {
        try {
            uint64_t chunk_no = 0, reads_so_far = 0;
            bool more = true;
            while (more && !failed) {
                const uint64_t t_r0 = now_us();
                auto c = std::make_shared<Chunk>();
                const uint64_t chunk_reads = chunk_no < (uint64_t)in_flight * n_dev ? chunk_reads_first : chunk_reads_max;
                c->no = chunk_no;
                c->first_read = reads_so_far;
                c->offsets.assign(1, 0);
                size_t bases = 0;
                auto admit = [&](InRecord&& r, bool copy) {
                    // Reads the device cannot take (longer than MAPAD_MAX_READ_LEN; the reference's limit is i16::MAX, src/map/record.rs:144-150) and empty
                    // reads stay in the output as unmapped records, so that input and output hold the same number of records.
                    const bool mappable = !r.seq.empty() && r.seq.size() <= MAPAD_MAX_READ_LEN;
                    if (!mappable) std::fprintf(stderr, "mapad-amd: read \"%s\" (%zu bp) is %s; written as unmapped\n", r.name.c_str(), r.seq.size(), r.seq.empty() ? "empty" : "longer than the device limit");
                    c->read_of.push_back(mappable ? (int64_t)(c->offsets.size() - 1) : -1);
                    if (mappable) {
                        if (copy) { c->seqs.append(r.seq.data(), r.seq.size()); c->quals.append(r.qual.data(), r.seq.size()); }
                        bases += r.seq.size();
                        c->offsets.push_back(bases);
                        c->flags.push_back(r.flags);
                    }
                    c->in.push_back(std::move(r));
                };
                std::vector<std::pair<uint32_t, uint32_t>> lines;
                const char* block = (merge_stage || clean_stage) ? nullptr : src.fastq_block(chunk_reads, lines);
                bool block_done = false;
                if (block && !lines.empty() && lines.size() % 4 == 0) {
                    // FASTQ fast path: the chunk's lines are cut sequentially (one memchr per line), the records are parsed by several threads
                    const size_t n_rec = lines.size() / 4;
                    std::vector<InRecord> recs(n_rec);
                    std::vector<char> good(n_rec, 0);
                    parallel_for(n_rec, host_threads, [&](size_t lo, size_t hi, unsigned) {
                        for (size_t i = lo; i < hi; ++i) good[i] = ReadSource::parse_fastq_record(block, &lines[4 * i], recs[i]);
                    });
                    bool all_good = true;
                    for (char g : good) all_good &= g != 0;
                    if (all_good) {
                        c->in.reserve(n_rec);
                        for (auto& r : recs) admit(std::move(r), false);
                        // bases of the mappable reads into the page-locked buffers, in parallel (offsets are known now)
                        c->seqs.append(nullptr, 0); c->quals.append(nullptr, 0);
                        c->seqs.resize_uninitialized(bases); c->quals.resize_uninitialized(bases);
                        parallel_for(c->in.size(), host_threads, [&](size_t lo, size_t hi, unsigned) {
                            for (size_t i = lo; i < hi; ++i) {
                                const int64_t k = c->read_of[i];
                                if (k < 0) continue;
                                const InRecord& r = c->in[i];
                                std::memcpy(c->seqs.p + c->offsets[(size_t)k], r.seq.data(), r.seq.size());
                                std::memcpy(c->quals.p + c->offsets[(size_t)k], r.qual.data(), r.seq.size());
                            }
                        });
                        more = lines.size() == 4 * chunk_reads;
                        block_done = true;
                    }
                }
                if (block && !block_done) {
                    // irregular text (blank lines, a malformed record, a truncated tail): the same lines through the tolerant sequential rules
                    size_t i = 0;
                    while (i < lines.size()) {
                        if (lines[i].second == 0) { ++i; continue; }
                        if (i + 4 > lines.size()) { if (lines.size() == 4 * chunk_reads) src.fastq_unread_from(lines[i].first); break; }  // a cut record goes back
                        InRecord r;
                        if (ReadSource::parse_fastq_record(block, &lines[i], r)) admit(std::move(r), true);
                        else std::fprintf(stderr, "Skip record due to an error: malformed FASTQ record\n");
                        i += 4;
                    }
                    more = lines.size() == 4 * chunk_reads;
                } else if (merge_stage) {
                    std::vector<InRecord> merged;
                    more = merge_stage->next_chunk(src, chunk_reads, merged);
                    for (auto& r : merged) admit(std::move(r), true);
                } else if (clean_stage) {
                    std::vector<InRecord> cleaned;
                    more = clean_stage->next_chunk(src, chunk_reads, cleaned);
                    for (auto& r : cleaned) admit(std::move(r), true);
                } else if (!block) {
                    InRecord r;
                    while (c->in.size() < chunk_reads && (more = src.next(r))) admit(std::move(r), true);
                }
                if (c->in.empty()) { if (more) continue; break; }  // a whole block of blank / malformed records: keep reading
                const uint64_t n_reads = c->offsets.size() - 1;
                c->slices.resize(n_dev);
                for (size_t d = 0; d < n_dev; ++d) {  // contiguous slices: concatenation in device order = input order
                    Slice& sl = c->slices[d];
                    const uint64_t base = n_reads / n_dev, extra = n_reads % n_dev;
                    sl.lo = d * base + std::min<uint64_t>(d, extra); sl.hi = sl.lo + base + (d < extra ? 1 : 0);
                    sl.offsets.resize(sl.hi - sl.lo + 1);
                    for (uint64_t i = sl.lo; i <= sl.hi; ++i) sl.offsets[i - sl.lo] = c->offsets[i] - c->offsets[sl.lo];
                }
                c->pending = (int)n_dev;
                us_reader += now_us() - t_r0;
                c->t_submit = std::chrono::steady_clock::now();
                for (size_t d = 0; d < n_dev; ++d) dev_q[d]->push(c);
                chunk_no += 1;
                reads_so_far += n_reads;
            }
        } catch (const std::exception& e) { fail(e.what()); }
        for (auto& q : dev_q) q->close();
    });

    // ---- device workers ----
    auto worker = [&](size_t d) {
        mapad_ctx_t* ctx = ctxs[d];
        auto submit = [&](const ChunkPtr& c) {
            const Slice& sl = c->slices[d];
            const uint64_t b0 = c->offsets[sl.lo];
            const uint64_t t0 = now_us();
            check(mapad_submit_batch(ctx, c->seqs.p + b0, c->quals.p + b0, sl.offsets.data(), sl.hi - sl.lo), "mapad_submit_batch");
            if (d == 0) us_submit += now_us() - t0;
        };
        auto coords = [&](const ChunkPtr& c) {
            Slice& sl = c->slices[d];
            const uint64_t t0 = now_us();
            // The device half of intervals_to_bam (reported hit, coordinates, XA candidates, X0 / X1) from the hits still resident on this GPU; the
            // strings and mapping qualities are the records thread's work, so that this thread goes straight back to submitting and fetching.
            // One seed per read of the run, whichever device maps it and however the input is cut into chunks: the run's seed advanced to the slice's first read.
            check(mapad_hits_to_coords_gpu(ctx, sl.res, mapad_records_seed_at(seed, c->first_read + sl.lo), &sl.coords), "mapad_hits_to_coords_gpu");
            if (d == 0) us_records += now_us() - t0;
        };
        auto finish = [&](const ChunkPtr& c) {
            if (--c->pending == 0) {
                c->per_read_s = std::chrono::duration<float>(std::chrono::steady_clock::now() - c->t_submit).count() / (float)std::max<size_t>(c->in.size(), 1);
                rec_q.push(c);
            }
        };
        auto records = [&](const ChunkPtr& c) { coords(c); finish(c); };
        auto collapse_count = [&](mapad_ctx_t* cx) {  // of the batch the context's accessors look at
            if (!collapse_duplicates) return;
            uint64_t info[8];
            check(mapad_last_collapse_info(cx, info), "mapad_last_collapse_info");
            n_collapse_reads += info[0]; n_collapse_groups += info[1];
        };
        auto collect = [&](const ChunkPtr& c, int age) -> bool {  // false: the hit pools were too small for this slice
            check(mapad_ctx_select_batch(ctx, age), "mapad_ctx_select_batch");
            const uint64_t t0 = now_us();
            const int rc = mapad_fetch_result(ctx, &c->slices[d].res);
            if (d == 0) us_fetch += now_us() - t0;
            if (rc == MAPAD_ERR_NOMEM) return false;
            check(rc, "mapad_fetch_result");
            collapse_count(ctx);
            return true;
        };
        auto rerun = [&](const ChunkPtr& c) {  // synchronous path that grows the pools
            const Slice& sl = c->slices[d];
            const uint64_t b0 = c->offsets[sl.lo];
            check(mapad_map_batch(ctx, c->seqs.p + b0, c->quals.p + b0, sl.offsets.data(), sl.hi - sl.lo, &c->slices[d].res), "mapad_map_batch");
            collapse_count(ctx);
        };
        try {
            std::deque<ChunkPtr> flying;  // submitted, oldest first
            // the oldest chunk's results; rare: a hit pool was too small — finish everything in flight, then repair synchronously, in order
            auto retire_oldest = [&] {
                if (collect(flying.front(), (int)flying.size() - 1)) { records(flying.front()); flying.pop_front(); return; }
                // (duplicates are marked in the order in which batches are converted, and the repair below converts out of input order)
                if (dedup_mode) throw std::runtime_error("a hit pool was too small for a batch while duplicates are marked: rerun with a smaller --batch_size");
                std::vector<bool> ok(flying.size(), false);
                for (size_t i = 1; i < flying.size(); ++i) ok[i] = collect(flying[i], (int)(flying.size() - 1 - i));
                // the coordinates of the collected ones first, while their hits and reads are on the device: a rerun launches over a batch slot (and the damage
                // profile, the coverage and the pileup count a batch only from there, once: neither dropped nor counted twice)
                for (size_t i = 0; i < flying.size(); ++i) if (ok[i]) coords(flying[i]);
                for (size_t i = 0; i < flying.size(); ++i) { if (!ok[i]) { rerun(flying[i]); coords(flying[i]); } finish(flying[i]); }
                flying.clear();
            };
            ChunkPtr c;
            while (dev_q[d]->pop(c)) {
                if (failed) continue;
                const uint64_t t_d0 = now_us();
                submit(c);  // the GPU starts on this chunk while older ones are collected and turned into records
                flying.push_back(c);
                c.reset();
                if ((int)flying.size() >= in_flight) retire_oldest();
                if (d == 0) us_device += now_us() - t_d0;
            }
            const uint64_t t_d1 = now_us();
            while (!flying.empty() && !failed) retire_oldest();
            if (d == 0) us_device += now_us() - t_d1;
        } catch (const std::exception& e) { fail(e.what()); }
        { ChunkPtr c; while (dev_q[d]->pop(c)) {} }  // after a failure: keep taking chunks so that the stage in front never blocks on a full queue (the process then exits non-zero)
    };
    std::vector<std::thread> workers;
    for (size_t d = 0; d < n_dev; ++d) workers.emplace_back(worker, d);

    // ---- records: the text half of intervals_to_bam (CIGAR / MD / XA strings, flags, mapping quality) on host threads, chunk by chunk in order ----
    std::thread recorder([&] {
        try {
            ChunkPtr c;
            while (rec_q.pop(c)) {
                if (failed) continue;
                const uint64_t t0 = now_us();
                for (auto& sl : c->slices) {
                    check(mapad_coords_to_records(idx, &prm, sl.res, c->flags.data() + sl.lo, sl.coords, &sl.recs), "mapad_coords_to_records");
                    mapad_coords_free(sl.coords); sl.coords = nullptr;
                }
                us_text += now_us() - t0;
                done_q.push(c);
            }
        } catch (const std::exception& e) { fail(e.what()); }
        { ChunkPtr c; while (rec_q.pop(c)) {} }  // see the device workers: a failed stage keeps draining its input
        done_q.close();
    });

    // ---- writer ----
    uint64_t n_total = 0, n_mapped = 0;
    uint64_t first_chunk_reads = 0, t_first_chunk_us = 0, t_last_chunk_us = 0;  // for the steady-state rate: everything behind the pipeline's fill (the first chunk's way through reader, device and writer)
    std::thread writer([&] {
        try {
            ChunkPtr c;
            while (done_q.pop(c)) {
                if (failed) continue;
                const uint64_t t_w0 = now_us();
                const size_t n = c->in.size();
                std::vector<std::vector<uint8_t>> enc(host_threads), comp(host_threads);
                std::vector<uint64_t> mapped(host_threads, 0);
                parallel_for(n, host_threads, [&](size_t lo, size_t hi, unsigned t) {
                    size_t d = 0;
                    for (size_t i = lo; i < hi; ++i) {
                        OutFields f;
                        const int64_t r = c->read_of[i];
                        if (r < 0) f.flags = (uint16_t)((c->in[i].flags & ~(0x8 | 0x20 | 0x2 | 0x100 | 0x800 | 0x10)) | 0x4);  // unmapped (mapping.rs:748-776)
                        else {
                            while ((uint64_t)r >= c->slices[d].hi) ++d;
                            const mapad_records_t* recs = c->slices[d].recs;
                            const mapad_record_t& m = recs->recs[(uint64_t)r - c->slices[d].lo];
                            f.mapped = m.mapped; f.reverse = m.reverse; f.flags = m.flags; f.tid = m.tid; f.pos = m.pos; f.mapq = m.mapq;
                            f.cigar.assign(recs->text + m.cigar_off, m.cigar_len); f.md.assign(recs->text + m.md_off, m.md_len); f.xa.assign(recs->text + m.xa_off, m.xa_len);
                            f.as = m.as_score; f.xs = m.xs_score; f.nm = m.nm; f.x0 = m.x0; f.x1 = m.x1; f.has_xs = m.has_xs; f.has_alt = m.mapped; f.xt = m.xt;
                            mapped[t] += m.mapped;
                            if (dscore_mode) {
                                const int32_t* score_q = nullptr; const uint8_t* scored = nullptr;
                                check(mapad_records_damage_scores(recs, &score_q, &scored), "mapad_records_damage_scores");
                                const uint64_t k = (uint64_t)r - c->slices[d].lo;
                                f.has_ds = scored && scored[k];
                                if (f.has_ds) f.ds = (float)score_q[k] / 256.0f;
                            }
                            if (rescale_mode && m.mapped) {  // QUAL of a mapped record: the rescaled qualities, at the slice's own offsets
                                const uint8_t* rq = nullptr; uint64_t n_rq = 0;
                                check(mapad_records_rescaled_quals(recs, &rq, &n_rq), "mapad_records_rescaled_quals");
                                const uint64_t k = (uint64_t)r - c->slices[d].lo, at = c->slices[d].offsets[k];
                                if (!rq || at + c->in[i].qual.size() > n_rq) throw std::runtime_error("the records carry no rescaled qualities");
                                f.rescaled = rq + at;
                            }
                        }
                        f.write_ds = dscore_mode != 0;
                        f.keep_oq = rescale_keep_oq;
                        f.xd = c->per_read_s;  // the reference stores the wall time of each read's search (mapping.rs:912-918); here: chunk time / reads
                        encode_bam_record(c->in[i], f, rg, enc[t]);
                    }
                    BgzfWriter::compress_all(enc[t].data(), enc[t].size(), comp[t]);  // every thread deflates what it encoded; the blocks are written in order below
                });
                for (unsigned t = 0; t < host_threads; ++t) { out.write_compressed(comp[t]); n_mapped += mapped[t]; }
                n_total += n;
                for (auto& sl : c->slices) { mapad_records_free(sl.recs); mapad_batch_result_free(sl.res); sl.recs = nullptr; sl.res = nullptr; }
                t_last_chunk_us = now_us();
                if (!t_first_chunk_us) { t_first_chunk_us = t_last_chunk_us; first_chunk_reads = n; }
                us_writer += now_us() - t_w0;
            }
        } catch (const std::exception& e) { fail(e.what()); }
        { ChunkPtr c; while (done_q.pop(c)) {} }
    });

    reader.join();
    for (auto& w : workers) w.join();
    rec_q.close();
    recorder.join();
    writer.join();
    if (failed) die(fail_msg);
    if (merge_stage) merge_stage->report(a, "map");
    if (clean_stage) clean_stage->report(a, "map");
    out.close();
    const double t_all = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    std::fprintf(stderr, "mapad-amd: %llu reads, %llu mapped; %zu device(s); index + contexts %.2f s, mapping %.2f s (%.0f reads/s)\n", (unsigned long long)n_total,
                 (unsigned long long)n_mapped, n_dev, t_load, t_all - t_load, (double)n_total / std::max(t_all - t_load, 1e-9));
    if (n_total > first_chunk_reads && t_last_chunk_us > t_first_chunk_us)  // the run without its fill: from the first chunk's records on disk to the last chunk's
        std::fprintf(stderr, "mapad-amd: steady state: %llu reads in %.2f s behind the first chunk (%.0f reads/s); pipeline fill %.2f s\n", (unsigned long long)(n_total - first_chunk_reads),
                     (t_last_chunk_us - t_first_chunk_us) * 1e-6, (double)(n_total - first_chunk_reads) / ((t_last_chunk_us - t_first_chunk_us) * 1e-6),
                     t_all - t_load - (t_last_chunk_us - t_first_chunk_us) * 1e-6);
    std::fprintf(stderr, "mapad-amd: stage busy time: reader %.2f s, device worker 0 %.2f s, writer %.2f s\n", us_reader.load() * 1e-6, us_device.load() * 1e-6, us_writer.load() * 1e-6);
    std::fprintf(stderr, "mapad-amd: device worker 0: submit %.2f s, fetch (incl. waiting for the GPU) %.2f s, coordinates %.2f s; records thread (strings, MAPQ) %.2f s\n",
                 us_submit.load() * 1e-6, us_fetch.load() * 1e-6, us_records.load() * 1e-6, us_text.load() * 1e-6);
    if (collapse_duplicates)
        std::fprintf(stderr, "mapad-amd: duplicate collapsing: %llu reads, %llu groups searched, %.1f %% of the reads collapsed\n", (unsigned long long)n_collapse_reads.load(),
                     (unsigned long long)n_collapse_groups.load(), 100.0 * (double)(n_collapse_reads.load() - n_collapse_groups.load()) / (double)std::max<uint64_t>(n_collapse_reads.load(), 1));
    st.report(a, idx, ctxs);
    for (auto* c : ctxs) mapad_ctx_destroy(c);
    mapad_index_free(idx);
    return 0;
}

// ---- `analyse`: the accumulator stages over an existing BAM, no search -----------------------------------------------------------------
// Every record's contig, POS, strand, CIGAR, MD:Z, X0 and AS go to mapad_ctx_accumulate_alignments with the read as sequenced; the stages count it as they would
// have behind the search that made it.  The base qualities a stage sees are QUAL; with --original_qualities the record's OQ:Z where it has one (what `map
// --rescale_keep_original` leaves of a rescaled record: the BAM then rescales to the same bytes).  Every record is a read: a secondary or supplementary record
// (0x100 / 0x800) without clips counts like any other.  The BAM's reference list must be the index's contigs.  One device, one batch at a time.
struct AlnTags {
    const uint8_t* md = nullptr; size_t md_len = 0;
    const uint8_t* oq = nullptr; size_t oq_len = 0;
    uint64_t x0 = 0;
    float as = 0.0f;
};
AlnTags aln_tags(const std::vector<uint8_t>& aux) {
    AlnTags t;
    for (size_t o = 0; o < aux.size();) {
        const size_t n = aux_field_size(aux.data() + o, aux.size() - o);
        if (!n) break;
        const uint8_t* p = aux.data() + o;
        int64_t v = 0;
        if (p[0] == 'M' && p[1] == 'D' && p[2] == 'Z') { t.md = p + 3; t.md_len = n - 4; }
        else if (p[0] == 'O' && p[1] == 'Q' && p[2] == 'Z') { t.oq = p + 3; t.oq_len = n - 4; }
        else if (p[0] == 'X' && p[1] == '0' && aux_int(p, v)) t.x0 = v > 0 ? (uint64_t)v : 0;
        else if (p[0] == 'A' && p[1] == 'S') { if (p[2] == 'f') std::memcpy(&t.as, p + 3, 4); else if (aux_int(p, v)) t.as = (float)v; }
        o += n;
    }
    return t;
}
// A record as it was read, with what the stages changed: the flags, QUAL (new_qual: the read's new qualities in read orientation, nullptr = as they are), and DS:f
// and OQ:Z as `map` writes them — an input DS / OQ dropped, the new one behind the other tags, DS first.  orig_qual: the qualities the stages saw, read orientation.
void encode_passthrough(const InRecord& in, uint16_t flags, const uint8_t* new_qual, const std::vector<uint8_t>& orig_qual, bool write_ds, bool has_ds, float ds, bool keep_oq,
                        std::vector<uint8_t>& out) {
    const std::vector<uint8_t>& b = in.raw;
    uint16_t n_cigar;
    uint32_t l_seq;
    std::memcpy(&n_cigar, &b[12], 2); std::memcpy(&l_seq, &b[16], 4);
    const size_t q_off = 32 + (size_t)b[8] + 4ull * n_cigar + (l_seq + 1) / 2, aux_off = q_off + l_seq;
    if (aux_off > b.size()) throw std::runtime_error("truncated BAM record");
    std::vector<uint8_t> rec(b.begin(), b.begin() + aux_off), oq;
    std::memcpy(&rec[14], &flags, 2);
    if (new_qual && l_seq && orig_qual.size() == l_seq) {
        if (std::memcmp(new_qual, orig_qual.data(), l_seq) != 0 && keep_oq) oq = orig_qual;
        std::vector<uint8_t> q(new_qual, new_qual + l_seq);
        if (in.flags & 0x10) { std::reverse(q.begin(), q.end()); std::reverse(oq.begin(), oq.end()); }
        std::copy(q.begin(), q.end(), rec.begin() + q_off);
    }
    for (size_t o = 0; o < in.aux.size();) {
        const size_t n = aux_field_size(in.aux.data() + o, in.aux.size() - o);
        if (!n) break;
        bool skip = write_ds && in.aux[o] == 'D' && in.aux[o + 1] == 'S';
        skip |= keep_oq && new_qual && in.aux[o] == 'O' && in.aux[o + 1] == 'Q';
        if (!skip) rec.insert(rec.end(), in.aux.begin() + o, in.aux.begin() + o + n);
        o += n;
    }
    if (write_ds && has_ds) { rec.push_back('D'); rec.push_back('S'); rec.push_back('f'); const uint8_t* p = (const uint8_t*)&ds; rec.insert(rec.end(), p, p + 4); }
    if (!oq.empty()) {  // Phred+33; a missing quality (255) has no printable form: '~'
        rec.push_back('O'); rec.push_back('Q'); rec.push_back('Z');
        for (uint8_t q : oq) rec.push_back(q <= 93 ? (uint8_t)(q + 33) : (uint8_t)'~');
        rec.push_back(0);
    }
    const uint32_t bs = (uint32_t)rec.size();
    const uint8_t* p = (const uint8_t*)&bs;
    out.insert(out.end(), p, p + 4);
    out.insert(out.end(), rec.begin(), rec.end());
}

int cmd_analyse(const Args& a, const std::vector<int>& devices, const std::string& cmdline) {
    for (const char* req : {"reads", "reference"}) if (!a.has(req)) die(std::string("analyse: --") + req + " is required");
    if (devices.size() != 1) die("analyse: one device only (--devices names more than one)");
    const std::string lib = a.get("library", "single_stranded");
    if (lib != "single_stranded" && lib != "double_stranded") die("analyse: --library must be single_stranded or double_stranded");
    const std::string mq = a.get("min_mapq", "0");
    if (mq.empty() || mq.find_first_not_of("0123456789") != std::string::npos || mq.size() > 3 || std::atoi(mq.c_str()) > 255) die("analyse: --min_mapq takes an integer 0..255");
    const uint32_t min_mapq = (uint32_t)std::atoi(mq.c_str());
    // the damage model of the stages that score with it (-f / -t / -d / -s / -D, --library); the search's own settings are not used: nothing is searched
    mapad_params_t prm;
    check(mapad_params_from_cli(&prm, lib == "single_stranded" ? MAPAD_LIBRARY_SINGLE_STRANDED : MAPAD_LIBRARY_DOUBLE_STRANDED, a.f("five_prime_overhang", 0),
                                a.f("three_prime_overhang", 0), a.f("ds_deamination_rate", 0), a.f("ss_deamination_rate", 0), a.f("divergence", 0.02f),
                                a.has("poisson_prob") ? a.f("poisson_prob", 0) : a.has("as_cutoff") ? -1.0f : 0.03f, a.f("as_cutoff", 0), a.f("as_cutoff_exponent", 1.0f),
                                a.f("indel_rate", 0.001f), a.f("gap_extension_penalty", 1.0f), std::atoi(a.get("gap_dist_ends", "5").c_str()),
                                std::atoi(a.get("max_num_gaps_open", "2").c_str()), a.flag("ignore_base_quality"), a.flag("no_search_limit_recovery"),
                                std::strtoull(a.get("chunk_size", "250000").c_str(), nullptr, 10)),
          "mapad_params_from_cli");
    const auto t_start = std::chrono::steady_clock::now();
    mapad_index_t* idx = nullptr;
    check(mapad_index_open(a.get("reference").c_str(), &idx), "mapad_index_open");
    const StageSetup st(a, idx, 1, "analyse");
    if (st.dscore_mode || st.rescale_mode || st.allele_mode) {  // these score with the damage model: as `map` does, its parameters are asked for, not defaulted
        for (const char* req : {"library", "five_prime_overhang", "ds_deamination_rate", "ss_deamination_rate"})
            if (!a.has(req)) die(std::string("analyse: --") + req + " is required by --damage_score, --rescale_qualities, --allele_likelihoods, --damage_consensus and --genotype_vcf");
        if (lib == "single_stranded" && !a.has("three_prime_overhang")) die("analyse: -t is required for single_stranded libraries by the stages that score with the damage model");
    }
    mapad_ctx_t* ctx = nullptr;
    check(mapad_ctx_create(idx, &prm, devices[0], &ctx), "mapad_ctx_create");
    check(mapad_ctx_set_fetch_d_arrays(ctx, 0), "mapad_ctx_set_fetch_d_arrays");
    st.apply(ctx);
    ReadSource src(a.get("reads"));
    if (!src.is_bam() || src.is_cram()) die("analyse: --reads takes a BAM whose mapped records carry MD:Z (FASTQ has no alignments; CRAM input is not supported here)");
    {   // a record's tid counts in the BAM's reference list: it must be the index's contigs, name for name and length for length
        const uint32_t n_ref = mapad_index_n_contigs(idx);
        if (src.refs().size() != n_ref) die("analyse: " + a.get("reads") + " names " + std::to_string(src.refs().size()) + " reference sequences, the index of " + a.get("reference") + " has " + std::to_string(n_ref));
        for (uint32_t i = 0; i < n_ref; ++i) {
            const char* name; uint64_t s, e;
            check(mapad_index_contig(idx, i, &name, &s, &e), "mapad_index_contig");
            if (src.refs()[i].first != name || src.refs()[i].second != e - s + 1)
                die("analyse: reference sequence " + std::to_string(i + 1) + " of " + a.get("reads") + " is " + src.refs()[i].first + " (" + std::to_string(src.refs()[i].second) + " bases), the index has " +
                    name + " (" + std::to_string(e - s + 1) + "): the BAM was not mapped against " + a.get("reference"));
        }
    }
    const bool writes = a.has("output");
    const bool use_oq = a.flag("original_qualities");
    src.keep_raw = writes;
    std::unique_ptr<BgzfWriter> out;
    if (writes) {
        out.reset(new BgzfWriter(a.get("output"), a.flag("force_overwrite")));
        std::string text = src.header_text();  // the input's header as it is, one @PG line added
        if (!text.empty() && text.back() != '\n') text.push_back('\n');
        std::string last_id;
        size_t same = 0;
        for (size_t i = 0; i < text.size();) {
            const size_t e = text.find('\n', i);
            const std::string line = text.substr(i, e - i);
            if (line.rfind("@PG", 0) == 0) {
                const size_t p = line.find("\tID:");
                if (p != std::string::npos) { const size_t q = line.find('\t', p + 4); last_id = line.substr(p + 4, q == std::string::npos ? std::string::npos : q - p - 4); }
                if (last_id == "mapAD.analyse" || last_id.rfind("mapAD.analyse.", 0) == 0) same += 1;
            }
            i = e + 1;
        }
        text += "@PG\tID:" + (same ? "mapAD.analyse." + std::to_string(same) : std::string("mapAD.analyse")) + "\tPN:mapAD\tVN:" + mapad_version() + "\tCL:" + cmdline +
                (last_id.empty() ? "" : "\tPP:" + last_id) + "\n";
        std::vector<uint8_t> h = {'B', 'A', 'M', 1};
        const uint32_t l_text = (uint32_t)text.size(), n_ref = mapad_index_n_contigs(idx);
        h.insert(h.end(), (const uint8_t*)&l_text, (const uint8_t*)&l_text + 4);
        h.insert(h.end(), text.begin(), text.end());
        h.insert(h.end(), (const uint8_t*)&n_ref, (const uint8_t*)&n_ref + 4);
        for (uint32_t i = 0; i < n_ref; ++i) {
            const char* name; uint64_t s, e;
            check(mapad_index_contig(idx, i, &name, &s, &e), "mapad_index_contig");
            const uint32_t l_name = (uint32_t)std::strlen(name) + 1, l_ref = (uint32_t)(e - s + 1);
            h.insert(h.end(), (const uint8_t*)&l_name, (const uint8_t*)&l_name + 4);
            h.insert(h.end(), name, name + l_name);
            h.insert(h.end(), (const uint8_t*)&l_ref, (const uint8_t*)&l_ref + 4);
        }
        out->write(h.data(), h.size());
    }
    static const char* const CLASS_NAME[MAPAD_ALN_CLASSES] = {"ok", "unmapped", "below_min_mapq", "no_md", "bad_contig", "unsupported_cigar", "length_mismatch", "md_mismatch", "off_contig"};
    uint64_t counts[MAPAD_ALN_CLASSES] = {}, n_total = 0, n_batches = 0, n_with_alignment = 0, n_without_md = 0, n_written = 0;
    double build_ms = 0.0;
    const uint64_t chunk_reads = std::max<uint64_t>(prm.chunk_size, 1);
    bool more = true;
    while (more) {
        std::vector<InRecord> in;
        std::vector<uint8_t> seqs, quals, md;
        std::vector<uint64_t> offsets{0};
        std::vector<uint32_t> cigar;
        std::vector<mapad_alignment_t> alns;
        InRecord r;
        while (in.size() < chunk_reads && (more = src.next(r))) {
            if (r.seq.size() > MAPAD_MAX_READ_LEN) die("analyse: read \"" + r.name + "\" is longer than the device limit");
            const AlnTags t = aln_tags(r.aux);
            mapad_alignment_t al{};
            al.tid = r.tid; al.pos0 = r.pos; al.flags = r.flags; al.mapq = r.mapq; al.x0 = t.x0; al.as_score = t.as;
            al.cigar_off = cigar.size(); al.n_cigar = (uint32_t)r.cigar.size(); al.md_off = md.size(); al.md_len = (uint32_t)t.md_len;
            cigar.insert(cigar.end(), r.cigar.begin(), r.cigar.end());
            if (t.md_len) md.insert(md.end(), t.md, t.md + t.md_len);
            const bool aligned = !(r.flags & 0x4) && r.tid >= 0;
            n_with_alignment += aligned; n_without_md += aligned && !t.md_len;
            seqs.insert(seqs.end(), r.seq.begin(), r.seq.end());
            if (use_oq && t.oq && t.oq_len == r.seq.size()) {  // --original_qualities: the qualities from before a rescaling, in the record's orientation
                std::vector<uint8_t> q(t.oq_len);
                for (size_t i = 0; i < t.oq_len; ++i) q[i] = (uint8_t)(t.oq[i] - 33);
                if (r.flags & 0x10) std::reverse(q.begin(), q.end());
                r.qual = q;
            }
            quals.insert(quals.end(), r.qual.begin(), r.qual.end());
            offsets.push_back(seqs.size());
            alns.push_back(al);
            in.push_back(std::move(r));
        }
        if (in.empty()) break;
        seqs.push_back(0); quals.push_back(0); cigar.push_back(0); md.push_back(0);  // (never read: the arrays have an address whatever the batch holds)
        mapad_aln_result_t* res = nullptr;
        check(mapad_ctx_accumulate_alignments(ctx, seqs.data(), quals.data(), offsets.data(), in.size(), alns.data(), cigar.data(), md.data(), min_mapq, &res),
              "mapad_ctx_accumulate_alignments");
        for (int k = 0; k < MAPAD_ALN_CLASSES; ++k) counts[k] += res->class_counts[k];
        build_ms += res->build_ms; n_total += in.size(); n_batches += 1;
        if (writes) {
            std::vector<uint8_t> enc;
            for (size_t i = 0; i < in.size(); ++i) {
                const bool dup = res->duplicate && res->duplicate[i];
                if (dup && st.dedup_mode == 2) continue;  // --exclude_duplicates: the record is dropped
                uint16_t flags = in[i].flags;
                if (st.dedup_mode) flags = (uint16_t)((flags & ~0x400) | (dup ? 0x400 : 0));
                const bool ok = res->status_class[i] == 0;
                const uint8_t* nq = st.rescale_mode && ok && res->rescaled_quals ? res->rescaled_quals + offsets[i] : nullptr;
                const bool has_ds = res->scored && res->scored[i];
                encode_passthrough(in[i], flags, nq, in[i].qual, st.dscore_mode != 0, has_ds, has_ds ? (float)res->score_q[i] / 256.0f : 0.0f, st.rescale_keep_oq, enc);
                n_written += 1;
            }
            out->write(enc.data(), enc.size());
        }
        mapad_aln_result_free(res);
    }
    if (n_with_alignment && n_without_md == n_with_alignment) {
        if (out) { out->close(); out.reset(); std::remove(a.get("output").c_str()); }  // nothing was counted: no output is left behind
        die("analyse: none of the " + std::to_string(n_with_alignment) + " mapped records of " + a.get("reads") + " carries an MD:Z tag (samtools calmd adds them)");
    }
    if (out) out->close();
    const double t_all = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    const double build_rate = build_ms > 0.0 ? (double)n_total / (build_ms * 1e-3) : 0.0;
    std::fprintf(stderr, "mapad-amd: analyse: %llu records in %llu batches, %llu counted (min MAPQ %u); track build %.3f ms (%.0f reads/s); %.2f s in all\n", (unsigned long long)n_total,
                 (unsigned long long)n_batches, (unsigned long long)counts[0], min_mapq, build_ms, build_rate, t_all);
    for (int k = 1; k < MAPAD_ALN_CLASSES; ++k)
        if (counts[k]) std::fprintf(stderr, "mapad-amd: analyse: %llu %s (seen, not counted)\n", (unsigned long long)counts[k], CLASS_NAME[k]);
    if (a.has("analyse_report"))
        write_lines(a.get("analyse_report"), [&](FILE* f) {
            std::fprintf(f, "#mapad-amd-analyse v1 min_mapq=%u\n", min_mapq);
            std::fprintf(f, "records\t%llu\n", (unsigned long long)n_total);
            for (int k = 0; k < MAPAD_ALN_CLASSES; ++k) std::fprintf(f, "%s\t%llu\n", CLASS_NAME[k], (unsigned long long)counts[k]);
            std::fprintf(f, "batches\t%llu\n", (unsigned long long)n_batches);
            if (writes) std::fprintf(f, "records_written\t%llu\n", (unsigned long long)n_written);
            std::fprintf(f, "track_build_ms\t%.3f\ntrack_build_reads_per_s\t%.0f\n", build_ms, build_rate);
        });
    st.report(a, idx, std::vector<mapad_ctx_t*>{ctx});
    mapad_ctx_destroy(ctx);
    mapad_index_free(idx);
    return 0;
}

// I/O self-test hook (no GPU needed): parse every input record and write it back as an unmapped BAM record
int cmd_recode(const Args& a) {
    ReadSource src(a.get("reads"));
    BgzfWriter out(a.get("output"), true);
    const std::string text = "@HD\tVN:1.6\tSO:unsorted\n";
    std::vector<uint8_t> h = {'B', 'A', 'M', 1};
    const uint32_t l_text = (uint32_t)text.size(), n_ref = 0;
    h.insert(h.end(), (const uint8_t*)&l_text, (const uint8_t*)&l_text + 4);
    h.insert(h.end(), text.begin(), text.end());
    h.insert(h.end(), (const uint8_t*)&n_ref, (const uint8_t*)&n_ref + 4);
    out.write(h.data(), h.size());
    InRecord r;
    std::vector<uint8_t> enc;
    while (src.next(r)) {
        OutFields f;
        f.flags = (uint16_t)((r.flags & ~(0x8 | 0x20 | 0x2 | 0x100 | 0x800 | 0x10)) | 0x4);
        enc.clear();
        encode_bam_record(r, f, a.get("read_group"), enc);
        out.write(enc.data(), enc.size());
    }
    out.close();
    return 0;
}


// ---- `worker`: the reference's `mapad worker --host H --port P` (src/distributed/worker.rs:35-236) with the search on a GPU --------------------
// Connects to a dispatcher, and for every TaskSheet it receives maps the records (k_mismatch_search per record: here one batch on the
// device) and answers with a ResultSheet: each record as it arrived, its hits in BinaryHeap array order, the time spent.  The first task
// names the index and carries the alignment parameters (worker.rs:57-75).  The dispatcher hands a worker one task at a time, so there
// is nothing to pipeline on this side.  Reads the device cannot take (empty, longer than MAPAD_MAX_READ_LEN) come back without hits.
// --dry_run answers every task with hit-less results without touching a GPU or an index (framing / codec check).
bool read_exact(int fd, uint8_t* p, size_t n) {  // false: the peer closed the connection before the first byte
    size_t got = 0;
    while (got < n) {
        const ssize_t k = ::read(fd, p + got, n - got);
        if (k == 0) { if (got == 0) return false; die("worker: connection closed inside a message"); }
        if (k < 0) { if (errno == EINTR) continue; die(std::string("worker: read: ") + std::strerror(errno)); }
        got += (size_t)k;
    }
    return true;
}

int cmd_worker(const Args& a, const std::vector<int>& devices) {
    const std::string host = a.get("host"), port = a.get("port", "3130");
    if (host.empty()) die("worker: --host is required");
    const bool dry = a.flag("dry_run");
    addrinfo hints{}, *ai = nullptr;
    hints.ai_family = AF_UNSPEC; hints.ai_socktype = SOCK_STREAM;
    if (getaddrinfo(host.c_str(), port.c_str(), &hints, &ai) != 0 || !ai) die("worker: cannot resolve " + host);
    int fd = -1;
    for (addrinfo* p = ai; p; p = p->ai_next) {
        fd = ::socket(p->ai_family, p->ai_socktype, p->ai_protocol);
        if (fd < 0) continue;
        if (::connect(fd, p->ai_addr, p->ai_addrlen) == 0) break;
        ::close(fd); fd = -1;
    }
    freeaddrinfo(ai);
    if (fd < 0) die("worker: cannot connect to " + host + ":" + port);
    mapad_index_t* idx = nullptr;
    mapad_ctx_t* ctx = nullptr;
    std::vector<uint8_t> msg;
    uint64_t n_tasks = 0, n_reads_total = 0;
    for (;;) {
        msg.resize(8);
        if (!read_exact(fd, msg.data(), 8)) break;  // the dispatcher has dropped the connection: done (worker.rs:203-206)
        uint64_t size; std::memcpy(&size, msg.data(), 8);
        // a task is at most one chunk of records (sequence + qualities + tags) plus the parameters: anything beyond a few GiB is a corrupt header,
        // not a task (the dispatcher sends chunk_size records, distributed/dispatcher.rs:223-247)
        if (size < 8 + 8 + 8 + 2 || size > (4ull << 30)) die("worker: implausible task size");
        try { msg.resize(size); } catch (const std::bad_alloc&) { die("worker: implausible task size (allocation failed)"); }
        if (!read_exact(fd, msg.data() + 8, size - 8)) die("worker: connection closed inside a message");
        const wire::Task t = wire::decode_task(msg.data(), msg.size());
        if (!dry && !idx) {  // worker.rs:57-65
            if (!t.has_reference) die("worker: the first task does not name the reference");
            check(mapad_index_open(t.reference_path.c_str(), &idx), "mapad_index_open");
        }
        if (!dry && !ctx) {  // worker.rs:67-75
            if (!t.has_params) die("worker: the first task carries no alignment parameters");
            check(mapad_ctx_create(idx, &t.params, devices[0], &ctx), "mapad_ctx_create");
            check(mapad_ctx_set_fetch_d_arrays(ctx, 0), "mapad_ctx_set_fetch_d_arrays");
            if (a.flag("collapse_duplicates")) check(mapad_ctx_set_collapse_duplicates(ctx, 1), "mapad_ctx_set_collapse_duplicates");
        }
        std::vector<int64_t> read_of(t.records.size(), -1);
        std::vector<uint8_t> seqs, quals;
        std::vector<uint64_t> offsets{0};
        for (size_t i = 0; i < t.records.size(); ++i) {
            const wire::RecordView& r = t.records[i];
            if (r.len == 0 || r.len > MAPAD_MAX_READ_LEN || r.qual_len != r.len) continue;
            read_of[i] = (int64_t)offsets.size() - 1;
            seqs.insert(seqs.end(), r.seq, r.seq + r.len); quals.insert(quals.end(), r.qual, r.qual + r.len);
            offsets.push_back(seqs.size());
        }
        const auto t0 = std::chrono::steady_clock::now();
        mapad_batch_result_t* res = nullptr;
        if (!dry) check(mapad_map_batch(ctx, seqs.data(), quals.data(), offsets.data(), offsets.size() - 1, &res), "mapad_map_batch");
        const double per_read = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / (double)std::max<size_t>(t.records.size(), 1);
        const std::vector<uint8_t> out = wire::encode_result(t, res, read_of, per_read);
        if (res) mapad_batch_result_free(res);
        for (size_t sent = 0; sent < out.size();) {
            const ssize_t k = ::write(fd, out.data() + sent, out.size() - sent);
            if (k < 0) { if (errno == EINTR) continue; die(std::string("worker: write: ") + std::strerror(errno)); }
            sent += (size_t)k;
        }
        n_tasks += 1; n_reads_total += t.records.size();
    }
    ::close(fd);
    std::fprintf(stderr, "mapad-amd worker: %llu task(s), %llu reads; the dispatcher closed the connection\n", (unsigned long long)n_tasks, (unsigned long long)n_reads_total);
    if (ctx) mapad_ctx_destroy(ctx);
    if (idx) mapad_index_free(idx);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    static const std::map<std::string, std::string> shorts = {
        {"-g", "reference"}, {"-r", "reads"}, {"-o", "output"}, {"-p", "poisson_prob"}, {"-c", "as_cutoff"}, {"-e", "as_cutoff_exponent"}, {"-l", "library"},
        {"-f", "five_prime_overhang"}, {"-t", "three_prime_overhang"}, {"-d", "ds_deamination_rate"}, {"-s", "ss_deamination_rate"}, {"-D", "divergence"},
        {"-i", "indel_rate"}, {"-x", "gap_extension_penalty"}, {"-R", "read_group"}, {"-1", "reads1"}, {"-2", "reads2"}, {"-k", "k"}};
    static const std::vector<std::string> bool_flags = {"ignore_base_quality", "no_search_limit_recovery", "force_overwrite", "host_index", "dry_run", "collapse_duplicates", "damage_profile_unique", "coverage_unique", "pileup_unique", "allele_unique", "mark_duplicates", "exclude_duplicates", "damage_score", "rescale_qualities", "rescale_pileup", "rescale_keep_original", "panel_unique", "original_qualities", "trim_adapter", "verify", "trim_poly_g", "trim_ns", "trim_qualities"};
    std::string cmdline, sub;
    for (int i = 0; i < argc; ++i) cmdline += std::string(i ? " " : "") + argv[i];
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k == "index" || k == "map" || k == "recode" || k == "worker" || k == "panel" || k == "analyse" || k == "merge" || k == "clean" || k == "mappability") { sub = k; continue; }
        if (k == "-v" || k == "-vv" || k == "-vvv") continue;
        if (k == "--batch_size") k = "--chunk_size";
        std::string key;
        if (shorts.count(k)) key = shorts.at(k);
        else if (k.rfind("--", 0) == 0) key = k.substr(2);
        else die("unexpected argument " + k);
        bool is_flag = false;
        for (auto& b : bool_flags) is_flag |= b == key;
        is_flag |= key == "host" && (sub == "merge" || sub == "clean" || sub == "mappability");  // `merge --host` / `mappability --host` is a switch (behind the subcommand); `worker --host H` names the dispatcher
        if (is_flag) a.flags.push_back(key);
        else { if (i + 1 >= argc) die("missing value for " + k); a.kv[key] = argv[++i]; }
    }
    // every chunk in flight has its own HIP stream; the runtime multiplexes streams onto 4 hardware queues unless told otherwise, and a
    // chunk's long tail would then hold back the launches queued behind it (must be set before the first HIP call)
    setenv("GPU_MAX_HW_QUEUES", "20", 0);
    const uint64_t seed = std::strtoull(a.get("seed", "1234").c_str(), nullptr, 10);
    const std::vector<int> devices = parse_devices(a.get("devices", a.get("device", "0")));
    try {
        if (sub == "index") return cmd_index(a, seed, devices[0]);
        if (sub == "map") return cmd_map(a, seed, devices, cmdline);
        if (sub == "recode") return cmd_recode(a);
        if (sub == "worker") return cmd_worker(a, devices);
        if (sub == "panel") return cmd_panel(a);
        if (sub == "analyse") return cmd_analyse(a, devices, cmdline);
        if (sub == "merge") return cmd_merge(a, devices[0]);
        if (sub == "clean") return cmd_clean(a, devices[0]);
        if (sub == "mappability") return cmd_mappability(a, devices[0]);
        die("usage: mapad-amd [--seed N] [--devices 0[,1,...|-7]] index|map|analyse|merge|clean|mappability|worker ...");
    } catch (const std::exception& e) { die(e.what()); }
}
