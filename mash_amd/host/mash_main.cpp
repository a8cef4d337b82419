// mash_main.cpp — `mash sketch | dist | triangle | cluster | info | paste | screen | taxscreen | bounds` on the MI355X hot path.
//
// Host C++ above the C ABI (include/mashgpu.h).  Option letters, defaults, file naming,
// stdout/stderr text and output order follow the reference commands
// (CommandSketch.cpp:36-169, CommandDistance.cpp:44-304, CommandTriangle.cpp:45-198,
// CommandInfo.cpp:40-299, CommandPaste.cpp:30-89, Command.cpp:165-200,311-347,
// sketchParameterSetup.cpp:15-125, Sketch.cpp:105-253).  All hashing / selection /
// comparison runs on the GPU through libmashgpu; there is no CPU fallback.
// Reads mode: -r, -m <copies>, -c <coverage>, -b <bytes>, -g, -M (exact, see mg_params::min_copies,
// ::bloom_bytes and mg_sketch_reads_host; the Bloom filter of -b has the geometry x86-64 builds of
// the reference use).
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <charconv>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <future>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mashgpu.h"
#include "fastx.h"
#include "msh_file.h"
#include "parse_pool.h"
#include "taxdb.h"
#include "../csrc/pvalue.h"
#include "../csrc/forest_key.h"

using std::cerr;
using std::cout;
using std::endl;
using std::string;
using std::vector;

namespace {

using hostpool::ParsedFile;
using hostpool::ParsePool;
using hostpool::Ref;
using hostpool::parse_file_concatenated;

const char *kSuffix = ".msh";
const char *kAlphabetNucleotide = "ACGT";
const char *kAlphabetProtein = "ACDEFGHIKLMNPQRSTVWY";

bool has_suffix(const string &s, const string &suf)
{
    return s.size() >= suf.size() && s.compare(s.size() - suf.size(), suf.size(), suf) == 0;
}

// ------------------------------------------------------------------------------- options
// Command::Option (Command.h:27-66): numbers are parsed with stof and kept as float.
struct Opt {
    enum Type { Boolean, Number, Integer, Size, File, String } type = Boolean;
    string id, def;
    float lo = 0, hi = 0;
    bool active = false;
    string arg;
    float num = 0;
};

struct Cmd {
    string name;
    std::map<string, Opt> opts;              // by long name
    std::map<string, string> by_id;
    vector<string> args;

    void add(const string &name_, Opt::Type t, const string &id, const string &def = "", float lo = 0, float hi = 0)
    {
        Opt o;
        o.type = t; o.id = id; o.def = def; o.lo = lo; o.hi = hi;
        opts[name_] = o;
        by_id[id] = name_;
        set_arg(opts[name_], def);
    }
    static void set_arg(Opt &o, string a)
    {
        o.arg = a;
        if (o.type == Opt::Number || o.type == Opt::Integer) {
            if (a.empty()) { o.num = 0; return; }
            bool failed = false;
            try {
                o.num = std::stof(a);
                if (o.lo != o.hi && (o.num < o.lo || o.num > o.hi)) failed = true;
                else if (o.type == Opt::Integer && (float)(uint64_t)o.num != o.num) failed = true;
            } catch (const std::exception &) { failed = true; }
            if (failed) {
                cerr << "ERROR: Argument to -" << o.id << " must be a" << (o.type == Opt::Integer ? "n integer" : " number");
                if (o.lo != o.hi) cerr << " between " << o.lo << " and " << o.hi;
                cerr << " (" << a << " given)" << endl;
                exit(1);
            }
        } else if (o.type == Opt::Size) {
            if (a.empty()) { o.num = 0; return; }
            char suffix = a[a.size() - 1];
            double factor = 1;
            if (suffix < '0' || suffix > '9') {
                switch (suffix) {
                    case 'k': case 'K': factor = 1e3; break;
                    case 'm': case 'M': factor = 1e6; break;
                    case 'g': case 'G': factor = 1e9; break;
                    case 't': case 'T': factor = 1e12; break;
                    default:
                        cerr << "ERROR: Unrecognized unit (\"" << suffix << "\") in argument to -" << o.id
                             << ". If specified, unit must be one of [kKmMgGtT]." << endl;
                        exit(1);
                }
                a.resize(a.size() - 1);
            }
            bool fail = false;
            try { o.num = std::stof(a); } catch (const std::exception &) { fail = true; }
            if (o.num <= 0 || (float)(uint64_t)o.num != o.num) fail = true;
            if (fail) {
                cerr << "ERROR: Argument to -" << o.id << " must be a whole number, optionally followed by one of [kKmMgGtT]." << endl;
                exit(1);
            }
            o.num = (float)(o.num * factor);
        }
    }
    // Command::run(argc, argv), Command.cpp:311-347
    int parse(int argc, const char **argv)
    {
        for (int i = 0; i < argc; i++) {
            if (argv[i][0] == '-' && argv[i][1] != 0) {
                if (!by_id.count(argv[i] + 1)) { cerr << "ERROR: Unrecognized option: " << argv[i] << endl; return 1; }
                Opt &o = opts.at(by_id.at(argv[i] + 1));
                o.active = true;
                if (o.type != Opt::Boolean) {
                    i++;
                    if (i == argc) { cerr << "ERROR: -" << o.id << " requires an argument" << endl; return 1; }
                    set_arg(o, argv[i]);
                }
            } else {
                args.push_back(argv[i]);
            }
        }
        return 0;
    }
    const Opt &o(const string &n) const { return opts.at(n); }
    bool has(const string &n) const { return opts.count(n) != 0; }
    void use_sketch_options()                  // Command::useSketchOptions, Command.cpp:354-379
    {
        add("threads", Opt::Integer, "p", "1");
        add("kmer", Opt::Integer, "k", "21", 1, 32);
        add("noncanonical", Opt::Boolean, "n");
        add("protein", Opt::Boolean, "a");
        add("alphabet", Opt::String, "z");
        add("case", Opt::Boolean, "Z");
        add("sketchSize", Opt::Integer, "s", "1000");
        add("individual", Opt::Boolean, "i");
        add("seed", Opt::Integer, "S", "42", 0, (float)0xFFFFFFFF);
        add("warning", Opt::Number, "w", "0.01", 0, 1);
        add("reads", Opt::Boolean, "r");
        add("memory", Opt::Size, "b");
        add("minCov", Opt::Integer, "m", "1");
        add("targetCov", Opt::Number, "c");
        add("genome", Opt::Size, "g");
    }
};

// ------------------------------------------------------------------------------- parameters
struct Params {                               // Sketch::Parameters (Sketch.h:34-106), fields used here
    int kmer = 0;
    uint64_t sketch_size = 0;
    uint32_t seed = 0;
    bool concatenated = false, noncanonical = false, preserve_case = false, reads = false, counts = false;
    float warning = 0;
    uint64_t genome_size = 0;
    uint32_t min_copies = 1;                  // minCov (-m)
    bool never_admit = false;                 // -m 0: the reference's heap admits no hash at all (an empty sketch)
    double target_cov = 0;                    // targetCov (-c)
    uint64_t bloom_bytes = 0;                 // memoryBound (-b)
    int threads = 1;                          // -p: files parsed concurrently (the GPU does the sketching)
    string alphabet;                          // normalised (uppercased unless preserve_case), sorted
    uint32_t alphabet_size = 0;
    bool use64 = false;
};

string normalise_alphabet(const string &chars, bool preserve_case)
{
    bool m[256] = {false};
    for (char c : chars) {
        char u = c;
        if (!preserve_case && u > 96 && u < 123) u -= 32;
        m[(unsigned char)u] = true;
    }
    string out;                               // Sketch::getAlphabetAsString: ascending byte order
    for (int i = 0; i < 256; i++) if (m[i]) out.push_back((char)i);
    return out;
}

void set_alphabet(Params &p, const string &chars)
{
    p.alphabet = normalise_alphabet(chars, p.preserve_case);
    p.use64 = mshio::use64_for(p.alphabet, p.preserve_case, (uint32_t)p.kmer, &p.alphabet_size);
}

// sketchParameterSetup, sketchParameterSetup.cpp:15-105
int sketch_parameter_setup(Params &p, const Cmd &c)
{
    p.kmer = (int)c.o("kmer").num;
    p.sketch_size = (uint64_t)c.o("sketchSize").num;
    p.concatenated = !c.o("individual").active;
    p.noncanonical = c.o("noncanonical").active;
    p.seed = (uint32_t)c.o("seed").num;
    p.reads = c.o("reads").active;
    p.preserve_case = c.o("case").active;
    p.threads = std::max(1, (int)c.o("threads").num);
    if (c.has("warning")) p.warning = c.o("warning").num;
    if (c.o("memory").active || c.o("minCov").active || c.o("targetCov").active) {
        if (c.o("memory").active && c.o("minCov").active) {          // sketchParameterSetup.cpp:44-48
            cerr << "ERROR: The option " << c.o("minCov").id << " cannot be used with " << c.o("memory").id << "." << endl;
            return 1;
        }
        if (c.o("memory").active) p.bloom_bytes = (uint64_t)c.o("memory").num;      // sketchParameterSetup.cpp:42
        p.reads = true;
        if (c.o("targetCov").active) p.target_cov = c.o("targetCov").num;          // sketchParameterSetup.cpp:24
        if (c.o("minCov").num >= 1) p.min_copies = (uint32_t)c.o("minCov").num;   // Sketch.cpp:1156 (reads mode only)
        // -m 0: multiplicityMinimum - 1 wraps (uint64_t), no pending count ever equals it, so the
        // reference's heap admits nothing (MinHashHeap.cpp:96-118): an empty sketch
        else if (c.o("minCov").active) p.never_admit = true;
    }
    if (c.o("genome").active) { p.reads = true; p.genome_size = (uint64_t)c.o("genome").num; }
    if (p.reads) p.counts = true;
    if (p.reads && c.o("threads").active)
        cerr << "WARNING: The option " << c.o("threads").id << " will be ignored with " << c.o("reads").id << "." << endl;
    if (p.reads && !p.concatenated) {
        cerr << "ERROR: The option " << c.o("individual").id << " cannot be used with " << c.o("reads").id << "." << endl;
        return 1;
    }
    if (c.o("protein").active) {
        p.noncanonical = true;
        if (!c.o("kmer").active) p.kmer = 9;
        set_alphabet(p, kAlphabetProtein);
    } else if (c.o("alphabet").active) {
        p.noncanonical = true;
        set_alphabet(p, c.o("alphabet").arg);
    } else {
        set_alphabet(p, kAlphabetNucleotide);
    }
    return 0;
}

void split_file(const string &file, vector<string> &lines)      // Command.cpp:398-414
{
    std::ifstream in(file);
    if (in.fail()) { cerr << "ERROR: Could not open " << file << ".\n"; exit(1); }
    string line;
    while (getline(in, line)) lines.push_back(line);
}

// ------------------------------------------------------------------------------- sketch set
struct SketchSet {                            // the part of class Sketch the commands use
    Params p;
    vector<Ref> refs;
    double kmer_space() const { return std::pow((double)p.alphabet_size, (double)p.kmer); }   // Sketch.cpp:509
};

// One device by default; more on request (MASH_GPU_DEVICES=all or "0,1,...", MASH_GPU_DEVICE=<n> picks the one):
// a local communicator -- one context per device, RCCL between them (MASH_GPU_DEVICES=all or a list;
// one device, device 0 or MASH_GPU_DEVICE, without it).  `ctx` is the first
// device's context: sketching and screening run there, `dist` and `triangle` shard their row
// blocks over all of them (mg_compare_*_sharded_host; the reference fans the same loops out to
// its -p threads, CommandTriangle.cpp:129-139, CommandDistance.cpp:195-232).
struct Gpu {
    mg_comm *comm = nullptr;
    mg_ctx *ctx = nullptr;
    Gpu()
    {
        vector<int> devs;
        if (const char *e = getenv("MASH_GPU_DEVICE")) devs.push_back(atoi(e));
        else if (const char *l = getenv("MASH_GPU_DEVICES")) {
            // "all": every visible GPU; else a comma separated list.  Without the variable ONE device is
            // used: more GPUs mean a communicator (RCCL start-up: seconds) that small jobs never earn
            // back, so the caller asks for them.
            if (strcmp(l, "all") == 0) {
                const int n = mg_device_count();
                for (int i = 0; i < n; i++) devs.push_back(i);
                l = "";
            }
            for (const char *q = l; *q;) {
                char *end;
                const long v = strtol(q, &end, 10);
                if (end == q) break;
                devs.push_back((int)v);
                q = *end == ',' ? end + 1 : end;
            }
        }
        if (devs.empty()) devs.push_back(0);
        if (mg_comm_create_local(devs.data(), (int)devs.size(), &comm) != MG_OK) {
            cerr << "ERROR: no usable GPU: " << mg_comm_last_error(nullptr) << endl;
            exit(1);
        }
        ctx = mg_comm_ctx(comm, 0);
    }
    ~Gpu() { mg_comm_destroy(comm); }
};

void params_from_header(Params &p, const mshio::Header &h)     // initParametersFromCapnp, Sketch.cpp:255-324
{
    p.kmer = (int)h.kmer_size;
    p.sketch_size = h.sketch_size;
    p.concatenated = h.concatenated;
    p.noncanonical = h.noncanonical;
    p.preserve_case = h.preserve_case;
    p.counts = h.has_counts;
    p.seed = h.seed;
    set_alphabet(p, h.has_alphabet ? h.alphabet : string(kAlphabetNucleotide));
}

// "Sketching <file>..." lines: one write(2) per file is what the consumer of 12 000 small genomes would
// spend a tenth of its time in.  Lines are gathered and written when 4 KiB have accumulated, before the
// consumer sleeps, and before anything else goes to stderr.
struct ProgressLog {
    string buf;
    void line(const string &l)
    {
        buf += l;
        if (buf.size() >= 4096) flush();
    }
    void flush()
    {
        if (buf.empty()) return;
        cerr << buf << std::flush;
        buf.clear();
    }
} g_progress;

// One batch of inputs -> GPU -> hash lists appended to `set`.
// Two modes: `stream` (files -> sketches): the bytes go to a mg_sketch_session as they are parsed --
// packed into pinned staging buffers and copied to the device while parsing goes on, no
// concatenated copy on the host; host mode (reads mode, whose -c replay needs the bytes): `bases`.
struct PendingBatch {
    vector<uint8_t> bases;
    vector<uint64_t> off{0};
    vector<Ref> refs;
    bool stream = false;
    mg_sketch_session *sess = nullptr;        // stream mode, created at the first byte (parameters are final by then)
    uint64_t nbytes = 0;
    // flush threshold in bytes: with parse workers the batches are SMALL, so that sketching, copying back and
    // handing out the hashes of one batch run while the workers parse the next (init_from_files)
    uint64_t max_bytes = 2ull << 30;
    // result buffers of mg_sketch_*: kept over the batches of a run (a fresh 100 MB vector is 25 000 page faults)
    std::unique_ptr<uint64_t[]> out_hashes;
    std::unique_ptr<uint32_t[]> out_nhash, out_counts;
    uint64_t out_cap = 0, out_cap_n = 0;
    // fn(0..n-1), possibly on several threads (the parse workers, when there are any)
    std::function<void(size_t, const std::function<void(size_t)> &)> parallel_for =
        [](size_t n, const std::function<void(size_t)> &fn) { for (size_t i = 0; i < n; i++) fn(i); };
    void append(const uint8_t *p, size_t n)
    {
        if (sess) {
            if (mg_sketch_add(sess, p, n) != MG_OK) { cerr << "ERROR: could not stage input for the GPU" << endl; exit(1); }
        } else {
            bases.insert(bases.end(), p, p + n);
        }
        nbytes += n;
    }
    void add_record(const string &seq)
    {
        append(reinterpret_cast<const uint8_t *>(seq.data()), seq.size());
        const uint8_t sep = (uint8_t)MG_RECORD_SEP;
        append(&sep, 1);
    }
    void end_sketch(Ref &&r)
    {
        if (sess) mg_sketch_end_sketch(sess);
        off.push_back(nbytes);
        refs.push_back(std::move(r));
    }
    void reset()
    {
        bases.clear();
        off.assign(1, 0);
        refs.clear();
        nbytes = 0;
    }
};

// MASH_AMD_TIMING=1: wall time of the stages of a run, to stderr at exit
struct StageClock {
    const bool on = getenv("MASH_AMD_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    vector<std::pair<string, double>> acc;
    void lap(const char *name)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        const double dt = std::chrono::duration<double>(t1 - t0).count();
        t0 = t1;
        for (auto &a : acc) if (a.first == name) { a.second += dt; return; }
        acc.emplace_back(name, dt);
    }
    ~StageClock()
    {
        if (!on) return;
        // (where the clock is declared before the Gpu -- sketch, screen -- the Gpu's destruction is in here; in triangle
        //  and cluster it is declared after it: the lap ends with the tables freed and the last lines written)
        lap("teardown");
        cerr << "timing:";
        for (auto &a : acc) cerr << ' ' << a.first << ' ' << a.second << " s;";
        cerr << endl;
    }
};

double g_gpu_sketch_seconds = 0;            // time inside mg_sketch_host (MASH_AMD_TIMING)

static mg_params batch_params(const SketchSet &set)
{
    mg_params mp;
    mg_params_init(&mp, set.p.kmer, set.p.sketch_size, set.p.seed, set.p.alphabet.c_str(), set.p.noncanonical,
                   set.p.preserve_case);
    if (set.p.reads) mp.min_copies = set.p.min_copies;
    return mp;
}

// stream mode: the session is opened when the first sketch of a batch arrives
void ensure_session(Gpu &gpu, const SketchSet &set, PendingBatch &b)
{
    if (!b.stream || b.sess) return;
    const mg_params mp = batch_params(set);
    if (mg_sketch_begin(gpu.ctx, &mp, &b.sess) != MG_OK) { cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); }
}

void flush_batch(Gpu &gpu, SketchSet &set, PendingBatch &b)
{
    if (b.refs.empty()) return;
    const mg_params mp = batch_params(set);
    const uint64_t n = b.refs.size(), s = set.p.sketch_size;
    if (n * s > b.out_cap || n > b.out_cap_n) {
        b.out_cap = std::max<uint64_t>(n * s, b.out_cap);
        b.out_cap_n = std::max<uint64_t>(n, b.out_cap_n);
        b.out_hashes.reset(new uint64_t[b.out_cap]);
        b.out_nhash.reset(new uint32_t[b.out_cap_n]);
        if (set.p.counts) b.out_counts.reset(new uint32_t[b.out_cap]);
    }
    uint64_t *hashes = b.out_hashes.get();
    uint32_t *nhash = b.out_nhash.get(), *counts = set.p.counts ? b.out_counts.get() : nullptr;
    if (!b.sess && b.bases.empty()) b.bases.push_back((uint8_t)MG_RECORD_SEP);
    const auto t_gpu = std::chrono::steady_clock::now();
    // (several GPUs, MASH_GPU_DEVICES: the batch is cut into byte-balanced blocks of sketches, one per device)
    const int sk_rc = b.sess ? mg_sketch_finish(b.sess, hashes, nhash, counts)
                      : mg_comm_size(gpu.comm) > 1 && mp.min_copies <= 1
                          ? mg_sketch_sharded_host(gpu.comm, &mp, b.bases.data(), b.bases.size(), b.off.data(), n, hashes, nhash, counts)
                          : mg_sketch_host(gpu.ctx, &mp, b.bases.data(), b.bases.size(), b.off.data(), n, hashes, nhash, counts);
    g_gpu_sketch_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_gpu).count();
    if (sk_rc != MG_OK) {
        g_progress.flush();
        const char *m = mg_comm_last_error(gpu.comm);
        cerr << "ERROR: " << ((m && *m) ? m : mg_last_error(gpu.ctx)) << endl;
        exit(1);
    }
    const size_t piece = 64;                                 // sketches per job
    b.parallel_for((n + piece - 1) / piece, [&](size_t j) {
        for (uint64_t i = j * piece; i < std::min<uint64_t>(n, (j + 1) * piece); i++) {
            b.refs[i].hashes.assign(hashes + i * s, hashes + i * s + nhash[i]);
            if (counts) b.refs[i].counts.assign(counts + i * s, counts + i * s + nhash[i]);
        }
    });
    for (uint64_t i = 0; i < n; i++) set.refs.push_back(std::move(b.refs[i]));
    b.reset();
}

const uint64_t kBatchBytes = 2ull << 30;
// ... and once it holds this many hash slots (sketches x sketch size): the hash, count and
// first-position arrays of a batch are n*s*8 + n*s*4 + n*s*8 bytes on the host and again on the
// device, so a file of a million short records at -s 10000 must not become one batch (the
// reference streams such a file in constant memory)
const uint64_t kBatchHashes = 1ull << 27;
static bool batch_full(const PendingBatch &b, uint64_t sketch_size)
{
    static const uint64_t cap = [] {                       // MASH_AMD_BATCH_HASHES: test knob
        const char *e = getenv("MASH_AMD_BATCH_HASHES");
        return e ? std::max<uint64_t>(1, strtoull(e, nullptr, 10)) : kBatchHashes;
    }();
    return b.nbytes > std::min(kBatchBytes, b.max_bytes) || (uint64_t)b.refs.size() * sketch_size > cap;
}

void queue_parsed_file(Gpu &gpu, SketchSet &set, PendingBatch &b, ParsedFile &&pf)
{
    if (!pf.error.empty()) { g_progress.flush(); cerr << pf.error << endl; exit(1); }
    ensure_session(gpu, set, b);
    b.append(pf.bases.data(), pf.bases.size());
    b.end_sketch(std::move(pf.ref));
    if (batch_full(b, set.p.sketch_size)) flush_batch(gpu, set, b);
}

// sketchFileBySequence (Sketch.cpp:326-370): one sketch per record
void queue_file_by_sequence(Gpu &gpu, SketchSet &set, PendingBatch &b, const string &file)
{
    fastx::Reader rd;
    if (!rd.open(file)) { cerr << "ERROR: could not open " << file << " for reading." << endl; exit(1); }
    fastx::Record rec;
    long l;
    while ((l = rd.next(rec)) >= 0) {
        if (l < set.p.kmer) continue;
        Ref ref;
        ref.name = rec.name;
        ref.comment = rec.comment;
        ref.length = (uint64_t)l;
        ensure_session(gpu, set, b);
        b.add_record(rec.seq);
        b.end_sketch(std::move(ref));
        if (batch_full(b, set.p.sketch_size)) flush_batch(gpu, set, b);
    }
    if (l != -1) { cerr << "\nERROR: reading " << file << "." << endl; exit(1); }
}

// Sketch::initFromReads -> sketchFile over all files, round robin (Sketch.cpp:96-103, :1147-1336)
// `shared`: a streamed-ingest session kept by the caller across calls (one reads-mode query file after the
// other in `mash dist -r`): its pinned staging buffers are allocated once, not per file
void sketch_reads(Gpu &gpu, SketchSet &set, const vector<string> &files, mg_sketch_session **shared = nullptr,
                  mg_reads_session **shared_reads = nullptr)
{
    vector<fastx::Reader *> readers;
    Ref ref;
    for (size_t f = 0; f < files.size(); f++) {
        if (files[f] == "-" && f > 1) { cerr << "ERROR: '-' for stdin must be first input" << endl; exit(1); }
        if (ref.name.empty() && files[f] != "-") ref.name = files[f];
        fastx::Reader *r = new fastx::Reader;
        if (!r->open(files[f])) { cerr << "ERROR: could not open " << files[f] << endl; exit(1); }
        readers.push_back(r);
    }
    PendingBatch b;
    // Every reads option goes through a reads session, chunk by chunk: the device hashes a chunk and hands
    // back the k-mers that can still change the heap, the host replays MinHashHeap::tryInsert over that
    // thinned stream (-m pending set, -b Bloom filter, -c stop test included) -- neither host nor device ever
    // holds more than a chunk or two, as the reference's reader loop holds one record and its heap
    // (Sketch.cpp:1196-1270).  With -c the reading STOPS with the chunk that reaches the target coverage
    // (Sketch.cpp:1258).  A chunk is on the device while the next one is being parsed.
    // MASH_AMD_READS_RESIDENT=1 (tests; plain -r / -m only): the round-2 route -- the reads leave for the device as
    // they are parsed and ONE sketch call runs over the whole read set in HBM at the end; same bytes out.
    const bool none = set.p.never_admit;          // -m 0: every record is read and counted, no hash is kept
    const bool must_replay = set.p.target_cov > 0 || set.p.bloom_bytes > 0;      // order-dependent by definition
    const bool cov_mode = !none && (must_replay || !getenv("MASH_AMD_READS_RESIDENT"));
    b.stream = !none && !cov_mode && !getenv("MASH_AMD_NO_STREAM");
    if (b.stream && shared) b.sess = *shared;
    ensure_session(gpu, set, b);
    mg_reads_session *rs = nullptr;
    size_t reads_chunk = 64u << 20;
    if (const char *e = getenv("MASH_AMD_READS_CHUNK")) reads_chunk = std::max<size_t>(1, strtoull(e, nullptr, 10));   // test knob
    int cov_stopped = 0;                          // written by this thread only, in wait_chunk
    int task_stopped = 0;                         // written by the task; read after its future.get()
    vector<uint8_t> in_flight;                    // the chunk the device is working on
    std::future<int> pending;
    auto wait_chunk = [&]() {
        if (!pending.valid()) return;
        if (pending.get() != MG_OK) { cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); }
        cov_stopped = task_stopped;
    };
    auto feed_chunk = [&]() {
        wait_chunk();                             // (cov_stopped now tells about the chunk before this one)
        if (b.bases.empty() || cov_stopped) { b.bases.clear(); return; }
        in_flight.swap(b.bases);
        b.bases.clear();
        pending = std::async(std::launch::async, [&]() { return mg_reads_add_host(rs, in_flight.data(), in_flight.size(), &task_stopped); });
    };
    if (cov_mode) {
        mg_params mp = batch_params(set);
        mp.min_copies = set.p.min_copies;
        mp.target_cov = set.p.target_cov;
        mp.bloom_bytes = set.p.bloom_bytes;
        // (MASH_AMD_SHARED_READS=1: one session for all reads-mode files of a run, emptied by mg_reads_reset between
        //  them -- its device buffers are then allocated once)
        if (shared_reads && *shared_reads) rs = *shared_reads;
        else if (mg_reads_begin(gpu.ctx, &mp, &rs) != MG_OK) { cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); }
        b.bases.reserve(std::min<size_t>(reads_chunk, 64u << 20) + (1u << 16));
    }
    fastx::Record rec;
    size_t it = 0;
    long l = -1;
    int count = 0;
    bool skipped = false;
    while (!readers.empty()) {
        l = readers[it]->next(rec);
        if (l < -1) break;
        if (l == -1) {
            delete readers[it];
            readers.erase(readers.begin() + it);
            if (it == readers.size()) it = 0;
            continue;
        }
        if (l >= set.p.kmer) {
            if (count == 0) {
                if (files[0] == "-") { ref.name = rec.name; ref.comment = rec.comment; }
                else ref.comment = rec.name + " " + rec.comment;
            }
            count++;
            if (!none) b.add_record(rec.seq);
            it++;
            if (it == readers.size()) it = 0;
            if (cov_mode && b.bases.size() >= reads_chunk) {
                feed_chunk();
                if (cov_stopped) { l = -1; break; }            // target coverage reached: the rest is not read
            }
        }
        else skipped = true;                                   // skipped without advancing to the next file (Sketch.cpp:1222-1226)
    }
    for (auto *r : readers) delete r;
    if (l != -1) { cerr << "\nERROR: reading input files." << endl; exit(1); }
    // (an empty result is refused below, once the length is known: Sketch.cpp:1302-1314)
    auto refuse_empty = [&]() {
        if (skipped) cerr << "\nWARNING: All fasta records in input files were shorter than the k-mer size (" << set.p.kmer << ")." << endl;
        else cerr << "\nERROR: Did not find fasta records in \"input files\"." << endl;
        exit(1);
    };
    if (count == 0 && set.p.genome_size == 0) refuse_empty();
    uint64_t reads_used = (uint64_t)count;
    auto wrap_comment = [&](uint64_t n) {                   // "[N seqs] first [...]" (Sketch.cpp:1284-1292)
        if (n > 1) ref.comment = "[" + std::to_string(n) + " seqs] " + ref.comment + " [...]";
    };
    if (cov_mode) {
        // the sequential heap, replayed exactly; with -c it also decided where reading stopped (Sketch.cpp:1258)
        feed_chunk();
        wait_chunk();
        const uint64_t s = set.p.sketch_size;
        vector<uint64_t> hashes(s);
        vector<uint32_t> counts(s);
        uint32_t nh = 0;
        if (mg_reads_finish(rs, hashes.data(), &nh, counts.data(), &reads_used) != MG_OK) {
            cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl;
            exit(1);
        }
        if (shared_reads && getenv("MASH_AMD_SHARED_READS")) { mg_reads_reset(rs); *shared_reads = rs; }
        else mg_reads_free(rs);
        ref.hashes.assign(hashes.begin(), hashes.begin() + nh);
        ref.counts.assign(counts.begin(), counts.begin() + nh);
        wrap_comment(reads_used);                              // the reference counts the reads it consumed
        set.refs.push_back(std::move(ref));
    } else if (none) {
        wrap_comment(reads_used);
        set.refs.push_back(std::move(ref));
    } else {
        wrap_comment(reads_used);
        b.end_sketch(std::move(ref));
        flush_batch(gpu, set, b);
    }
    if (b.sess && shared) *shared = b.sess;               // empty again after its finish: the next file fills it
    else if (b.sess) mg_sketch_session_free(b.sess);
    Ref &r = set.refs.back();
    // estimateSetSize (MinHashHeap.h:45): 2^bits * n / max kept hash
    double est = 0;
    if (!r.hashes.empty())
        est = std::pow(2.0, set.p.use64 ? 64.0 : 32.0) * (double)r.hashes.size() / (double)r.hashes.back();
    r.length = set.p.genome_size ? set.p.genome_size : (uint64_t)est;
    // nothing kept (e.g. -m 2 on a genome without repeats) and no -g: length 0 is "no records" (Sketch.cpp:1302-1314)
    if (r.length == 0) refuse_empty();
    cerr << "Estimated genome size: " << est << endl;
    double msum = 0;                                       // estimateMultiplicity (MinHashHeap.h:44)
    for (uint32_t c : r.counts) msum += c;
    cerr << "Estimated coverage:    " << (r.counts.empty() ? 0.0 : msum / (double)r.counts.size()) << endl;
    if (set.p.target_cov > 0) cerr << "Reads used:            " << reads_used << endl;      // Sketch.cpp:1324-1327
}

// the .msh branch of Sketch::initFromFiles (Sketch.cpp:120-172) + loadCapnp
bool load_msh_into(SketchSet &set, const string &file, bool first_sets_params, bool contain = false)
{
    mshio::File hdr;
    vector<uint8_t> image;                                       // read once, parsed twice (header, then lists)
    string e = mshio::load_file(file, image);
    if (e.empty()) e = mshio::parse_msh(image.data(), image.size(), hdr, true, 0);
    if (!e.empty()) { cerr << "ERROR: " << e << endl; exit(1); }
    if (first_sets_params) params_from_header(set.p, hdr.header);
    Params t;
    params_from_header(t, hdr.header);
    if (set.p.alphabet != t.alphabet) {
        cerr << "\nWARNING: The sketch file " << file << " has different alphabet (" << t.alphabet << ") than the current alphabet (" << set.p.alphabet << "). This file will be skipped." << endl << endl;
        return false;
    }
    if (t.seed != set.p.seed) {
        cerr << "\nWARNING: The sketch " << file << " has a seed size (" << t.seed << ") that does not match the current seed (" << set.p.seed << "). This file will be skipped." << endl << endl;
        return false;
    }
    if (t.kmer != set.p.kmer) {
        cerr << "\nWARNING: The sketch " << file << " has a kmer size (" << t.kmer << ") that does not match the current kmer size (" << set.p.kmer << "). This file will be skipped." << endl << endl;
        return false;
    }
    if (!contain && t.sketch_size < set.p.sketch_size) {
        cerr << "\nWARNING: The sketch file " << file << " has a target sketch size (" << t.sketch_size << ") that is smaller than the current sketch size (" << set.p.sketch_size << "). This file will be skipped." << endl << endl;
        return false;
    }
    if (t.noncanonical != set.p.noncanonical) {
        cerr << "\nWARNING: The sketch file " << file << " is " << (t.noncanonical ? "noncanonical" : "canonical") << ", which is incompatible with the current setting. This file will be skipped." << endl << endl;
        return false;
    }
    if (t.sketch_size > set.p.sketch_size)
        cerr << "\nWARNING: The sketch file " << file << " has a target sketch size (" << t.sketch_size << ") that is larger than the current sketch size (" << set.p.sketch_size << "). Its sketches will be reduced." << endl << endl;
    mshio::File f;
    e = mshio::parse_msh(image.data(), image.size(), f, false, set.p.sketch_size);
    if (!e.empty()) { cerr << "ERROR: " << e << endl; exit(1); }
    for (auto &r : f.references) {
        Ref x;
        x.name = std::move(r.name);
        x.comment = std::move(r.comment);
        x.length = r.length;
        x.hashes = std::move(r.hashes);
        x.counts = std::move(r.counts);
        set.refs.push_back(std::move(x));
    }
    return true;
}

bool parseable_by_pool(const vector<string> &files, size_t i, const Params &p)
{
    return p.concatenated && !(p.reads && p.concatenated) && !has_suffix(files[i], kSuffix) && files[i] != "-";
}

// A run of parsed files goes to the device as ONE window of the session's pinned staging buffer
// (mg_sketch_stage): the copies into it are dealt to the parse workers, the consumer only keeps the books.
void queue_parsed_group(Gpu &gpu, SketchSet &set, PendingBatch &b, vector<ParsedFile> &group, ParsePool &pool)
{
    ensure_session(gpu, set, b);
    uint64_t total = 0;
    for (const ParsedFile &pf : group) total += pf.bases.size();
    uint8_t *win = nullptr;
    if (mg_sketch_stage(b.sess, total, &win) != MG_OK) { g_progress.flush(); cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); }
    vector<ParsePool::Copy> jobs;
    uint64_t at = 0;
    for (const ParsedFile &pf : group) {
        // (pieces of <= 1 MiB, so that one large genome is copied by several workers too)
        for (uint64_t o = 0; o < pf.bases.size(); o += 1 << 20)
            jobs.push_back({win + at + o, pf.bases.data() + o, (size_t)std::min<uint64_t>(1 << 20, pf.bases.size() - o)});
        at += pf.bases.size();
    }
    pool.copy_all(jobs);
    for (ParsedFile &pf : group) {
        if (mg_sketch_commit(b.sess, pf.bases.size()) != MG_OK) { g_progress.flush(); cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); }
        b.nbytes += pf.bases.size();
        b.end_sketch(std::move(pf.ref));
    }
    group.clear();
    if (batch_full(b, set.p.sketch_size)) flush_batch(gpu, set, b);
}

void init_from_files(Gpu &gpu, SketchSet &set, const vector<string> &files, const Params &p, int verbosity = 1,
                     bool enforce_parameters = false, ParsePool *early = nullptr, bool contain = false)
{
    set.p = p;
    PendingBatch b;
    mg_sketch_session *reads_sess = nullptr;               // shared by the reads-mode query files
    mg_reads_session *reads_rs = nullptr;
    // (env: the concatenate-then-copy path, for tests; several GPUs: whole batches, cut over the devices)
    b.stream = !getenv("MASH_AMD_NO_STREAM") && mg_comm_size(gpu.comm) <= 1;
    // concatenated mode with -p > 1: files are parsed ahead by a pool of workers (ParsePool)
    // Reads options (-r -m -c -b -g) reach sketchFile through here too (`mash dist -r ref.msh reads.fq`,
    // `mash triangle -r ...`): ONE sketch per file with the reads-mode heap, the estimated (or -g)
    // genome size as its length and the two "Estimated ..." lines (Sketch.cpp:1156, :1272-1282,
    // :1320-1330) -- the same code path as `mash sketch -r` over that one file.
    const bool reads_files = set.p.reads && set.p.concatenated;
    auto parseable = [&](size_t i) { return parseable_by_pool(files, i, set.p); };
    std::unique_ptr<ParsePool> own;
    ParsePool *pool = early;
    if (!pool && p.threads > 1 && !reads_files) { own.reset(new ParsePool(files, (size_t)p.threads, parseable)); pool = own.get(); }
    const bool grouped = pool && b.stream && !getenv("MASH_AMD_NO_GROUPS");
    if (pool) {
        b.parallel_for = [pool](size_t n, const std::function<void(size_t)> &fn) { pool->run_jobs(n, fn); };
        if (b.stream) {
            const char *e = getenv("MASH_AMD_BATCH_BYTES");
            b.max_bytes = e ? std::max<uint64_t>(1, strtoull(e, nullptr, 10)) : 64ull << 20;
        }
    }
    vector<ParsedFile> group;
    auto announce = [&](size_t i) {
        if (verbosity <= 0) return;
        if (files[i] == "-") g_progress.line("Sketching from stdin...\n");
        else g_progress.line("Sketching " + files[i] + "...\n");
    };
    for (size_t i = 0; i < files.size(); i++) {
        if (has_suffix(files[i], kSuffix)) {
            g_progress.flush();
            flush_batch(gpu, set, b);                      // keep input order
            load_msh_into(set, files[i], i == 0 && !enforce_parameters, contain);
            if (pool) pool->skip(i);
            continue;
        }
        announce(i);
        if (pool && parseable(i)) {
            // (a worker opens the file; a failure comes back in input order as the file's error)
            if (pool->ready_bytes(i) < 0) g_progress.flush();          // about to wait: show where we are
            ParsedFile pf = pool->take(i, set.p.kmer);
            if (grouped) ensure_session(gpu, set, b);
            const uint64_t cap = grouped ? mg_sketch_stage_capacity(b.sess) : 0;
            if (!grouped || !pf.error.empty() || pf.bases.size() > cap) {
                queue_parsed_file(gpu, set, b, std::move(pf));
                continue;
            }
            // this file and those behind it that are parsed already, while they fit one staging window
            uint64_t bytes = pf.bases.size();
            group.push_back(std::move(pf));
            while (i + 1 < files.size() && group.size() < 4096 && parseable(i + 1)) {
                const long long nb = pool->ready_bytes(i + 1);
                if (nb < 0 || bytes + (uint64_t)nb > cap) break;
                ParsedFile nx = pool->take(i + 1, set.p.kmer);
                announce(++i);
                if (!nx.error.empty()) {                   // everything before it first, then its message (and exit)
                    queue_parsed_group(gpu, set, b, group, *pool);
                    queue_parsed_file(gpu, set, b, std::move(nx));
                }
                bytes += (uint64_t)nb;
                group.push_back(std::move(nx));
            }
            queue_parsed_group(gpu, set, b, group, *pool);
            continue;
        }
        g_progress.flush();
        if (files[i] != "-") {
            FILE *t = fopen(files[i].c_str(), "r");
            if (!t) { cerr << "ERROR: could not open " << files[i] << " for reading." << endl; exit(1); }
            fclose(t);
        }
        if (pool) pool->skip(i);
        if (reads_files) {
            flush_batch(gpu, set, b);                      // keep input order
            sketch_reads(gpu, set, {files[i]}, &reads_sess, &reads_rs);
        } else if (set.p.concatenated) {
            queue_parsed_file(gpu, set, b, parse_file_concatenated(files[i], set.p.kmer));
        } else {
            queue_file_by_sequence(gpu, set, b, files[i]);
        }
    }
    g_progress.flush();
    flush_batch(gpu, set, b);
    if (b.sess) mg_sketch_session_free(b.sess);
    if (reads_sess) mg_sketch_session_free(reads_sess);
    if (reads_rs) mg_reads_free(reads_rs);
}

string write_set(SketchSet &set, const string &path, bool consume = false)
{
    mshio::File f;
    f.header.kmer_size = (uint32_t)set.p.kmer;
    f.header.sketch_size = (uint32_t)set.p.sketch_size;
    f.header.seed = set.p.seed;
    f.header.concatenated = set.p.concatenated;
    f.header.noncanonical = set.p.noncanonical;
    f.header.preserve_case = set.p.preserve_case;
    f.header.has_alphabet = true;
    f.header.alphabet = set.p.alphabet;
    f.header.has_counts = set.p.counts;
    f.references.reserve(set.refs.size());
    for (Ref &r : set.refs) {
        mshio::Reference x;
        x.name = r.name; x.comment = r.comment; x.length = r.length;
        if (consume) { x.hashes = std::move(r.hashes); x.counts = std::move(r.counts); }     // (the caller is done with the set)
        else { x.hashes = r.hashes; x.counts = r.counts; }
        f.references.push_back(std::move(x));
    }
    return mshio::write_msh(path, f);
}

// warnKmerSize machinery (CommandSketch.cpp:110-131, sketchParameterSetup.cpp:107-125, Sketch.cpp:53-61)
struct KmerWarning {
    uint64_t length_max = 0;
    string name;
    double random_chance = 0;
    int k_min = 0;
    int count = 0;
};

KmerWarning scan_kmer_warning(const SketchSet &set)
{
    KmerWarning w;
    const double warning = set.p.warning;
    const double threshold = (warning * set.kmer_space()) / (1. - warning);
    for (const Ref &r : set.refs) {
        if ((double)r.length > threshold) {
            if (w.count == 0 || r.length > w.length_max) {
                w.length_max = r.length;
                w.name = r.name;
                w.random_chance = 1. / (set.kmer_space() / r.length + 1.);
                w.k_min = (int)std::ceil(std::log(r.length * (1 - warning) / warning) / std::log((double)set.p.alphabet_size));
            }
            w.count++;
        }
    }
    return w;
}

void warn_kmer_size(const SketchSet &set, const KmerWarning &w)
{
    cerr << "\nWARNING: For the k-mer size used (" << set.p.kmer << "), the random match probability (" << w.random_chance
         << ") is above the specified warning threshold (" << set.p.warning << ") for the sequence \"" << w.name
         << "\" of size " << w.length_max;
    if (w.count > 1) cerr << " (and " << (w.count - 1) << " others)";
    cerr << ". Distances to " << (w.count == 1 ? "this sequence" : "these sequences")
         << " may be underestimated as a result. To meet the threshold of " << set.p.warning << ", a k-mer size of at least "
         << w.k_min << " is required. See: -k, -w." << endl << endl;
}

// the sharded calls record their error in the communicator, the calls on one context in that context
int report_error(Gpu &gpu)
{
    const char *m = mg_comm_last_error(gpu.comm);
    cerr << "ERROR: " << ((m && *m) ? m : mg_last_error(gpu.ctx)) << endl;
    return 1;
}

// dense table upload
// the same table on EVERY device of the communicator (host -> GPU 0 -> RCCL broadcast); rows: only those sketches, in that order
mg_dtable *upload_all(Gpu &gpu, const SketchSet &set, uint64_t s, vector<uint64_t> *lengths_out = nullptr, bool by_rows = false,
                      const vector<uint32_t> *rows = nullptr)
{
    const uint64_t n = rows ? rows->size() : set.refs.size();
    vector<uint64_t> h(std::max<uint64_t>(n * s, 1), MG_HASH_PAD), len(std::max<uint64_t>(n, 1));
    vector<uint32_t> nh(std::max<uint64_t>(n, 1));
    for (uint64_t i = 0; i < n; i++) {
        const Ref &r = set.refs[rows ? (*rows)[i] : i];
        const uint64_t k = std::min<uint64_t>(r.hashes.size(), s);
        nh[i] = (uint32_t)k;
        len[i] = r.length;
        std::copy(r.hashes.begin(), r.hashes.begin() + k, h.begin() + i * s);
    }
    mg_dtable *d = nullptr;
    // by_rows: the larger side of a rect job -- every GPU gets a block of its rows instead of a replica
    if ((by_rows ? mg_dtable_upload_rows(gpu.comm, h.data(), nh.data(), len.data(), n, s, &d)
                 : mg_dtable_upload(gpu.comm, h.data(), nh.data(), len.data(), n, s, &d)) != MG_OK)
        exit(report_error(gpu));
    if (lengths_out) *lengths_out = len;
    return d;
}

// ------------------------------------------------------------------------------- commands
int cmd_sketch(int argc, const char **argv)
{
    Cmd c;
    c.name = "sketch";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    c.add("prefix", Opt::File, "o");
    c.add("id", Opt::File, "I");
    c.add("comment", Opt::File, "C");
    c.add("counts", Opt::Boolean, "M");
    c.use_sketch_options();
    if (c.parse(argc, argv)) return 1;
    if (c.args.empty() || c.o("help").active) {
        cout << "\nUsage:\n\n  mash sketch [options] <input> [<input>] ...\n\n"
                "Create a sketch file (.msh) from fasta/fastq inputs (gzipped or not) on the GPU.\n"
                "Options: -l -o <prefix> -I <id> -C <comment> -p <threads> -k <1-32> -s <size> -S <seed> -i -n -a -z <alphabet> -Z -w <p>\n"
                "Reads:   -r  -m <min copies> (0 keeps no hash, as in the reference: refused unless -g gives a length)  -c <target coverage>\n"
                "         -b <Bloom filter bytes, K/M/G/T>  -g <genome size>  -M (store multiplicities)\n\n";
        return 0;
    }
    Params p;
    p.counts = c.o("counts").active;
    if (sketch_parameter_setup(p, c)) return 1;
    vector<string> files;
    for (const string &a : c.args) { if (c.o("list").active) split_file(a, files); else files.push_back(a); }
    if ((c.o("id").active || c.o("comment").active) && files.size() > 1 && !p.reads)
        cerr << "WARNING: -I and -C will only apply to first sketch" << endl;
    StageClock clk;
    // MASH_AMD_EARLY_PARSE=1: the parse workers start BEFORE the device context exists, so that its creation
    // (0.07-0.2 s) is spent parsing (bounded: MASH_AMD_PARSE_AHEAD bytes, default 1 GiB).  Off by default:
    // measured (tools/sketch_e2e.py, 12 000 x 50 kbp at -p 16: 0.26 s with, 0.21 s without) -- once the
    // consumer's chain (staging copies, device tail, hand-out) is what bounds the run, parsing earlier buys
    // nothing and a gigabyte of parse buffers allocated up front slows context creation and the writer.
    // Not when a leading .msh may still change k (Sketch.cpp:140-160).
    std::unique_ptr<ParsePool> early;
    if (!p.reads && p.concatenated && p.threads > 1 && !files.empty() && !has_suffix(files[0], kSuffix) && getenv("MASH_AMD_EARLY_PARSE")) {
        early.reset(new ParsePool(files, (size_t)p.threads, [&files, &p](size_t i) { return parseable_by_pool(files, i, p); }));
        early->start(0, p.kmer);
    }
    Gpu gpu;
    clk.lap("device");
    SketchSet set;
    if (p.reads) { set.p = p; sketch_reads(gpu, set, files); }
    else init_from_files(gpu, set, files, p, 1, false, early.get());
    early.reset();
    clk.lap("ingest+sketch");
    if (clk.on) cerr << "timing: of which mg_sketch_host " << g_gpu_sketch_seconds << " s" << endl;
    if (c.o("id").active && !set.refs.empty()) set.refs[0].name = c.o("id").arg;
    if (c.o("comment").active && !set.refs.empty()) set.refs[0].comment = c.o("comment").arg;
    const KmerWarning w = scan_kmer_warning(set);
    string prefix = !c.o("prefix").arg.empty() ? c.o("prefix").arg : (c.args[0] == "-" ? string("stdin") : c.args[0]);
    if (!has_suffix(prefix, kSuffix)) prefix += kSuffix;
    cerr << "Writing to " << prefix << "..." << endl;
    const string e = write_set(set, prefix, true);
    clk.lap("write");
    if (!e.empty()) { cerr << "ERROR: " << e << endl; return 1; }
    if (w.count > 0 && !p.reads) warn_kmer_size(set, w);
    return 0;
}

// Bulk result lines: same bytes `cout << double` would print (default precision 6 == "%g" ==
// to_chars general/6), but buffered and without a flush per line -- at 10^8 lines the
// reference's `<< endl` formatting is what a run waits for once the kernels take milliseconds.
struct FastOut {
    string buf;
    bool sink;                               // false: a worker's piece, appended to the real one in order
    explicit FastOut(bool to_stdout = true) : sink(to_stdout) { if (sink) buf.reserve(1u << 22); }
    ~FastOut() { if (sink) flush(); }
    void flush()
    {
        cout.flush();
        if (!buf.empty()) { fwrite(buf.data(), 1, buf.size(), stdout); fflush(stdout); buf.clear(); }
    }
    void room() { if (sink && buf.size() > (1u << 22) - 4096) flush(); }
    FastOut &operator<<(const string &x) { buf += x; return *this; }
    FastOut &operator<<(const char *x) { buf += x; return *this; }
    FastOut &operator<<(char x) { buf += x; return *this; }
    FastOut &operator<<(double v)
    {
        char t[40];
        auto r = std::to_chars(t, t + sizeof t, v, std::chars_format::general, 6);
        buf.append(t, r.ptr);
        return *this;
    }
    FastOut &operator<<(uint32_t v)
    {
        char t[16];
        auto r = std::to_chars(t, t + sizeof t, v);
        buf.append(t, r.ptr);
        return *this;
    }
    FastOut &operator<<(uint64_t v)
    {
        char t[24];
        auto r = std::to_chars(t, t + sizeof t, v);
        buf.append(t, r.ptr);
        return *this;
    }
    void eol() { buf += '\n'; room(); }
};

// Text of a block of result rows, formatted on worker threads and written in row order (number
// formatting, not the GPU, bounds a full matrix: ~50 ns per value on one core).  Rows are cut
// into chunks of >= 2^17 pairs, a wave of chunks is formatted concurrently, the pieces are
// appended in order; fn(out, row, slot) must only touch slot-private state besides `out`.
unsigned emit_threads()
{
    static const unsigned nt = []() {
        if (const char *e = getenv("MASH_AMD_EMIT_THREADS")) return (unsigned)std::min(64, std::max(1, atoi(e)));
        return std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    }();
    return nt;
}

template <class CostFn, class RowFn>
void emit_rows(FastOut &out, uint64_t r0, uint64_t r1, CostFn cost, RowFn fn)
{
    const unsigned nt = emit_threads();
    vector<uint64_t> cut{r0};
    uint64_t acc = 0;
    for (uint64_t r = r0; r < r1; r++) {
        acc += cost(r);
        if (acc >= (1u << 17)) { cut.push_back(r + 1); acc = 0; }
    }
    if (cut.back() != r1) cut.push_back(r1);
    const size_t nchunks = cut.size() - 1;
    if (nt < 2 || nchunks < 2) {
        for (uint64_t r = r0; r < r1; r++) fn(out, r, 0u);
        return;
    }
    vector<FastOut> part;
    part.reserve(nt);
    for (unsigned t = 0; t < nt; t++) part.emplace_back(false);
    for (size_t c0 = 0; c0 < nchunks; c0 += nt) {
        const unsigned m = (unsigned)std::min<size_t>(nt, nchunks - c0);
        vector<std::thread> th;
        for (unsigned t = 0; t < m; t++)
            th.emplace_back([&, t]() {
                part[t].buf.clear();
                for (uint64_t r = cut[c0 + t]; r < cut[c0 + t + 1]; r++) fn(part[t], r, t);
            });
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < m; t++) { out.buf += part[t].buf; out.room(); }
    }
}

// One line of `mash dist` (writeOutput, CommandDistance.cpp:247-304)
inline void print_pair_line(FastOut &out, const Ref &ref, const Ref &qry, bool comment, uint32_t numer, uint32_t denom, double distance, double p)
{
    out << ref.name;
    if (comment) out << ':' << ref.comment;
    out << '\t' << qry.name;
    if (comment) out << ':' << qry.comment;
    out << '\t' << distance << '\t' << p << '\t' << numer << '/' << denom;
    out.eol();
}
template <class Rec>                          // mg_pair, mg_result
inline void print_pair_line(FastOut &out, const Ref &ref, const Ref &qry, bool comment, const Rec &r) { print_pair_line(out, ref, qry, comment, r.numer, r.denom, r.distance, r.p_value); }

// One line of `mash triangle -E` (CommandTriangle.cpp:159-198)
inline void print_edge_line(FastOut &out, const string &row_label, const string &col_label, uint32_t numer, uint32_t denom, double distance, double p)
{
    out << row_label << '\t' << col_label << '\t' << distance << '\t' << p << '\t' << numer << '/' << denom;
    out.eol();
}

// Thresholded runs (-d < 1 or -v < 1): both filters of compareSketches, the distances and p-values
// of the survivors and their compaction run on the device (mg_compare_*_results_host), so only
// surviving pairs cross PCIe, as finished records; bit-identical to the host arithmetic
// (MASH_AMD_NO_FILTER=1 takes the full-matrix path instead, MASH_AMD_HOST_FINISH=1 the host tail).
bool edge_filter_wanted(double d_max, double p_max) { return (d_max < 1.0 || p_max < 1.0) && !getenv("MASH_AMD_NO_FILTER"); }
bool host_finish_wanted() { return getenv("MASH_AMD_HOST_FINISH") != nullptr; }

// A list result (mg_result, mg_edge) of unknown length: a second call once the library has said how long it is
template <class T, class Call>
bool fetch_list(Gpu &gpu, vector<T> &v, Call call)
{
    uint64_t n = 0;
    if (v.size() < (1u << 16)) v.resize(1u << 16);
    int rc = call(v.data(), (uint64_t)v.size(), &n);
    if (rc == MG_ERR_NOMEM && n > v.size()) {
        v.resize(n);
        rc = call(v.data(), (uint64_t)v.size(), &n);
    }
    if (rc != MG_OK) { report_error(gpu); return false; }
    v.resize(n);
    return true;
}

bool finish_edge(const mg_edge &e, uint64_t len_ref, uint64_t len_qry, int k, double kspace, double p_max, mg_pair &pr)
{
    pr.numer = e.numer;
    pr.denom = e.denom;
    pr.distance = mg_distance(e.numer, e.denom, k);
    pr.p_value = mg_p_value(e.numer, len_ref, len_qry, kspace, e.denom);
    pr.pass = pr.p_value <= p_max;                           // CommandDistance.cpp:419-422
    return pr.pass;
}

// MASH_AMD_BLOCK_PAIRS=<n> (for tests): no route's block budget is larger than n, so that a small input crosses
// block boundaries.  It can only lower a budget; read once per process.
uint64_t block_budget(uint64_t budget)
{
    static const char *e = getenv("MASH_AMD_BLOCK_PAIRS");
    static const uint64_t knob = e ? std::max<uint64_t>(1, strtoull(e, nullptr, 10)) : ~0ull;
    return std::min(knob, budget);
}

// The row blocks [r0, r1) of a compare and their pair counts: of a triangle (ncols == 0: row i has i pairs) or of a
// rectangle (every row has ncols).  A block always takes its first row; a row is added while the sum stays within the
// budget.  for (Blocks b(begin, end, budget, ncols); b.next();) ...
struct Blocks {
    const uint64_t end, ncols, budget;
    uint64_t r0, r1, npairs = 0;
    Blocks(uint64_t begin, uint64_t end_, uint64_t budget_, uint64_t ncols_ = 0)
        : end(end_), ncols(ncols_), budget(block_budget(budget_)), r0(begin), r1(begin) {}
    bool next()
    {
        r0 = r1;
        npairs = 0;
        while (r1 < end && (npairs == 0 || (ncols ? npairs + ncols : npairs + r1) <= budget)) { npairs += ncols ? ncols : r1; r1++; }
        return r0 < r1;
    }
};

// Budgets of a block of rows whose survivors alone come back (the library cuts its own device blocks): triangle, rectangle
const uint64_t kTriFilteredPairs = 1ull << 31, kDistFilteredPairs = 1ull << 30;

// The pairs within d_max from one context's tables, block by block: of a triangle (rows 1 .. n of t) or of a rectangle (the nq
// rows of qry against the nref of ref).  The p-value filter stays with the caller (finish_edge): use(edges) gets every block's
// list.  Non-zero: an error has been reported.
template <class Use>
int tri_edge_blocks(Gpu &gpu, const mg_table *t, uint64_t n, int kmer, double d_max, Use use)
{
    vector<mg_edge> edges;
    for (Blocks b(1, n, kTriFilteredPairs); b.next();) {
        if (!fetch_list(gpu, edges, [&](mg_edge *o, uint64_t cap, uint64_t *cnt) {
                return mg_compare_tri_filter_host(gpu.ctx, t, b.r0, b.r1, kmer, d_max, o, cap, cnt); }))
            return 1;
        use(edges);
    }
    return 0;
}
template <class Use>
int rect_edge_blocks(Gpu &gpu, const mg_table *ref, const mg_table *qry, uint64_t nref, uint64_t nq, int kmer, double d_max, Use use)
{
    vector<mg_edge> edges;
    for (Blocks b(0, nq, kDistFilteredPairs, nref); b.next();) {
        if (!fetch_list(gpu, edges, [&](mg_edge *o, uint64_t cap, uint64_t *cnt) {
                return mg_compare_rect_filter_host(gpu.ctx, ref, qry, b.r0, b.r1, kmer, d_max, o, cap, cnt); }))
            return 1;
        use(edges);
    }
    return 0;
}

// -N on the host (MASH_AMD_HOST_FINISH=1): appends the `keep` nearest of one row's passing pairs {row, neighbour, ...} to
// res, in the order of mg_compare_*_topk_host: by shared hashes as an exact fraction, equal fractions by neighbour index
void select_nearest(vector<mg_result> &row, uint64_t keep, vector<mg_result> &res)
{
    const size_t take = std::min<size_t>(row.size(), keep);
    std::partial_sort(row.begin(), row.begin() + (ptrdiff_t)take, row.end(), [](const mg_result &a, const mg_result &b) {
        const uint64_t l = (uint64_t)a.numer * (b.denom ? b.denom : 1u), r = (uint64_t)b.numer * (a.denom ? a.denom : 1u);
        return l > r || (l == r && a.col < b.col);
    });
    res.insert(res.end(), row.begin(), row.begin() + (ptrdiff_t)take);
}

// The distances of one (s, k) as text: a distance depends on (numer, denom) alone, and nearly every pair has denom == s,
// so a cell "\t<distance>" is formatted once per numerator, not per pair.  A distance above d_max is an empty cell
// (`dist -t`, CommandDistance.cpp:409-412).
struct DistText {
    uint64_t s = 0;
    int kmer = 0;
    double d_max = HUGE_VAL;
    vector<string> txt;                       // empty: no table, cell() is not to be called
    void build(uint64_t s_, int kmer_, double d_max_ = HUGE_VAL)
    {
        s = s_; kmer = kmer_; d_max = d_max_;
        txt.resize(s + 1);
        for (uint64_t x = 0; x <= s; x++) {
            FastOut t(false);
            put(t, mg_distance((uint32_t)x, (uint32_t)s, kmer));
            txt[x] = t.buf;
        }
    }
    bool on() const { return !txt.empty(); }
    void put(FastOut &o, double d) const { o << '\t'; if (!(d > d_max)) o << d; }
    void cell(FastOut &o, uint32_t numer, uint32_t denom) const
    {
        if (denom == s) o << txt[numer];
        else put(o, mg_distance(numer, denom, kmer));
    }
};

// "Max p-value" of `mash triangle`: the peak over finished blocks, and within a block one running peak per emit_rows slot.
// The Phylip matrix prints distances only, and of the p-values just the largest (to stderr).
// A distance depends on (numer, denom) alone -> one table per run; and a p-value can only raise
// the peak if even the pair of the two longest genomes sharing that many hashes would: the
// p-value grows with both lengths (larger r in CommandDistance.cpp:437-441, the binomial tail
// grows with r), so pairs whose bound stays below the running peak skip the incomplete-beta
// evaluation.  The bound test has a 1e-9 relative margin for the rounding of that evaluation.
struct PeakPValue {
    double peak = 0;
    vector<double> slot;
    uint64_t s = 0, l1 = 0, l2 = 0;           // the sketch size the bound holds for, the two largest lengths
    double kspace = 0;
    vector<double> bound;                     // NaN: not evaluated yet
    // (the bounds are evaluated on first use: a run meets a few hundred distinct numerators, and an
    //  exact tail costs O(x) -- all s of them up front were minutes at s = 10^5 and a large r)
    void use_bound(const vector<uint64_t> &lengths, uint64_t s_, double kspace_)
    {
        s = s_; kspace = kspace_;
        for (uint64_t v : lengths) { if (v > l1) { l2 = l1; l1 = v; } else if (v > l2) l2 = v; }
        bound.assign(s + 1, std::nan(""));
    }
    // p-value of the two longest genomes sharing x hashes, with a 1e-9 margin; memoised (workers may both
    // evaluate an entry: they store the same bits)
    double bound_of(uint32_t x)
    {
        uint64_t bits = __atomic_load_n(reinterpret_cast<const uint64_t *>(&bound[x]), __ATOMIC_RELAXED);
        double v;
        memcpy(&v, &bits, 8);
        if (v != v) {                                              // not evaluated yet
            v = mg_p_value(x, l1, l2, kspace, s) * (1.0 + 1e-9);
            memcpy(&bits, &v, 8);
            __atomic_store_n(reinterpret_cast<uint64_t *>(&bound[x]), bits, __ATOMIC_RELAXED);
        }
        return v;
    }
    void begin() { slot.assign(emit_threads(), peak); }          // a block starts from what earlier blocks established
    // a pair of the lean writers (use_bound): evaluated only if its p-value could raise the slot's peak
    void note(double &slot_peak, uint32_t numer, uint32_t denom, uint64_t len_i, uint64_t len_j)
    {
        if (denom != s || bound_of(numer) >= slot_peak) {
            const double pv = mg_p_value(numer, len_i, len_j, kspace, denom);
            if (pv > slot_peak) slot_peak = pv;
        }
    }
    void merge() { for (double v : slot) if (v > peak) peak = v; }
};

// the inputs of a command from argument `first` on; with -l every argument is a file of file names
vector<string> input_files(const Cmd &c, size_t first = 0)
{
    vector<string> files;
    for (size_t i = first; i < c.args.size(); i++) { if (c.o("list").active) split_file(c.args[i], files); else files.push_back(c.args[i]); }
    return files;
}

// A table on the devices.  Declared after the Gpu, so that it is freed before mg_comm_destroy runs.
struct DTableFree { void operator()(mg_dtable *d) const { mg_dtable_free(d); } };
using DTable = std::unique_ptr<mg_dtable, DTableFree>;

// what every compare command ends with
int finish_run(const SketchSet &set, const KmerWarning &w, bool reads) { if (w.count > 0 && !reads) warn_kmer_size(set, w); return 0; }

// Options that cannot be given together, for `dist` and `triangle`: the first row that matches is the one reported.  Non-zero: refused.
struct OptionClash { const char *a, *b; };
int refuse_clashes(const Cmd &c, std::initializer_list<OptionClash> clashes)
{
    for (const OptionClash &x : clashes) {
        if (!c.o(x.a).active || !c.o(x.b).active) continue;
        cerr << "ERROR: The option -" << c.o(x.a).id << " cannot be used with -" << c.o(x.b).id << "." << endl;
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------- -H: the distance spectrum
// `triangle -H` / `dist -H`: instead of the pairs that pass -d and -v, the distinct shared-hashes fractions among them and how many
// pairs have each (include/mashgpu.h: mg_compare_tri_spectrum_host) -- one line per bin, nearest first:
//   <distance> TAB <numer>/<denom> TAB <pairs> TAB <pairs at or below this distance>
// The bins are counted on the device, block of rows by block of rows; bins of equal key are added here.
// MASH_AMD_HOST_FINISH=1 is the host route, which the tests judge the device route by: with a filter on the records of
// mg_compare_*_results_host are binned here; with the filters off the pairs that share a hash (mg_compare_*_sparse_host) are, and
// every other pair is {0, min(s, |A| + |B|)} by the rule stated there.
struct Spectrum {
    std::map<uint64_t, uint64_t> bins;        // numer << 32 | denom -> pairs
    void add(uint32_t numer, uint32_t denom, uint64_t n = 1) { if (n) bins[(uint64_t)numer << 32 | denom] += n; }
    // the pairs of one row with clamped hash count c against rows whose clamped counts are histogrammed in `below`: all {0, rule
    // denominator} until the listed ones are taken out again (unlist)
    void add_rule(uint64_t s, uint64_t c, const std::map<uint64_t, uint64_t> &below)
    {
        for (const auto &h : below) add(0, (uint32_t)std::min(s, c + h.first), h.second);
    }
    void unlist(uint64_t s, uint64_t ca, uint64_t cb) { bins[std::min(s, ca + cb)]--; }
    void print(FastOut &out, int kmer) const
    {
        vector<std::pair<uint64_t, uint64_t>> v;
        for (const auto &b : bins) if (b.second) v.push_back(b);
        // ascending distance: descending fraction, exactly; 0/0 (distance 0) as 1/1; equal fractions by ascending denominator
        std::sort(v.begin(), v.end(), [](const std::pair<uint64_t, uint64_t> &a, const std::pair<uint64_t, uint64_t> &b) {
            const uint64_t ad = (uint32_t)a.first, bd = (uint32_t)b.first;
            const uint64_t l = (ad ? a.first >> 32 : 1) * (bd ? bd : 1), r = (bd ? b.first >> 32 : 1) * (ad ? ad : 1);
            return l != r ? l > r : ad < bd;
        });
        uint64_t below = 0;
        for (const auto &b : v) {
            const uint32_t numer = (uint32_t)(b.first >> 32), denom = (uint32_t)b.first;
            below += b.second;
            out << mg_distance(numer, denom, kmer) << '\t' << numer << '/' << denom << '\t' << b.second << '\t' << below;
            out.eol();
        }
    }
};

// ------------------------------------------------------------------------------- dist
// Budgets of a block of query rows (MASH_AMD_BLOCK_PAIRS lowers them; kDistFilteredPairs stands with rect_edge_blocks):
const uint64_t kDistFullPairs = 1ull << 24;         // the whole matrix comes back: 512 MiB of mg_pair per block
const uint64_t kDistNearestRecords = 1ull << 22;    // -N: `keep` records per query, 128 MiB of mg_result per block

struct DistRun {
    Gpu &gpu;
    const SketchSet &ref, &qry;
    const bool table, comment;
    const uint32_t nearest;
    const double d_max, p_max, kspace;
    const int kmer;
    const uint64_t nref, nq;
    vector<uint64_t> len_ref, len_qry;
    DTable dr, dq;
    mg_table *tr, *tq;                        // device 0's replicas: what the host-tail test routes address
    vector<mg_counts> counts;                 // (these keep their capacity over the blocks)
    vector<mg_pair> pairs;
    FastOut out;
    DistRun(Gpu &g, const SketchSet &r, const SketchSet &q, bool table_, bool comment_, uint32_t nearest_, double d_max_, double p_max_, bool ref_by_rows)
        : gpu(g), ref(r), qry(q), table(table_), comment(comment_), nearest(nearest_), d_max(d_max_), p_max(p_max_), kspace(r.kmer_space()),
          kmer(r.p.kmer), nref(r.refs.size()), nq(q.refs.size()), dr(upload_all(g, r, r.p.sketch_size, &len_ref, ref_by_rows)),
          dq(upload_all(g, q, q.p.sketch_size, &len_qry)), tr(mg_dtable_local(dr.get(), 0)), tq(mg_dtable_local(dq.get(), 0)) {}
};

// the counts of a block of query rows x all references; with finish (MASH_AMD_HOST_FINISH=1) distances, p-values and filters
// of those on the host
int dist_counts(DistRun &r, const Blocks &b, bool finish)
{
    r.counts.resize(b.npairs);
    if (mg_compare_rect_sharded_host(r.gpu.comm, r.dr.get(), r.dq.get(), b.r0, b.r1, r.counts.data()) != MG_OK) return report_error(r.gpu);
    if (finish) {
        r.pairs.resize(b.npairs);
        mg_finish_rect_host(r.counts.data(), r.len_ref.data(), r.nref, r.len_qry.data() + b.r0, b.r1 - b.r0, r.kmer, r.kspace, r.d_max, r.p_max, r.pairs.data());
    }
    return 0;
}

void dist_emit_results(DistRun &r, const vector<mg_result> &res)
{
    emit_rows(r.out, 0, res.size(), [](uint64_t) { return 1; }, [&](FastOut &o, uint64_t x, unsigned) {
        const mg_result &e = res[x];
        print_pair_line(o, r.ref.refs[e.col], r.qry.refs[e.row], r.comment, e);
    });
}

// -N: per query its nearest references, ranked and cut on the device (mg_compare_rect_topk_sharded_host): N records per
// query cross PCIe.
int dist_nearest(DistRun &r)
{
    const uint64_t keep = std::min<uint64_t>(r.nearest, r.nref);
    vector<mg_result> res, row;
    if (!host_finish_wanted()) {
        for (Blocks b(0, r.nq, kDistNearestRecords, keep); b.next();) {
            if (res.size() < b.npairs) res.resize(b.npairs);                            // the largest possible answer: one call
            if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_rect_topk_sharded_host(r.gpu.comm, r.dr.get(), r.dq.get(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.nearest, o, cap, n); }))
                return 1;
            dist_emit_results(r, res);
        }
        return 0;
    }
    // MASH_AMD_HOST_FINISH=1: the matrix of counts, the host tail, and the same selection here
    for (Blocks b(0, r.nq, kDistFullPairs, r.nref); b.next();) {
        if (dist_counts(r, b, true)) return 1;
        res.clear();
        for (uint64_t q = b.r0; q < b.r1; q++) {
            const mg_pair *pr = r.pairs.data() + (q - b.r0) * r.nref;
            row.clear();                                        // the query's passing pairs as {query, reference, ...}
            for (uint64_t x = 0; x < r.nref; x++)
                if (pr[x].pass) row.push_back(mg_result{(uint32_t)q, (uint32_t)x, pr[x].numer, pr[x].denom, pr[x].distance, pr[x].p_value});
            select_nearest(row, keep, res);
        }
        dist_emit_results(r, res);
    }
    return 0;
}

// -d / -v without -t: the surviving pairs as finished records
int dist_filtered(DistRun &r)
{
    if (host_finish_wanted())
        // MASH_AMD_HOST_FINISH=1: the pairs within -d from device 0's replicas, p-values and the -v filter here
        return rect_edge_blocks(r.gpu, r.tr, r.tq, r.nref, r.nq, r.kmer, r.d_max, [&](const vector<mg_edge> &edges) {
            emit_rows(r.out, 0, edges.size(), [](uint64_t) { return 1; }, [&](FastOut &o, uint64_t x, unsigned) {
                const mg_edge &e = edges[x];
                mg_pair pr;
                if (finish_edge(e, r.len_ref[e.col], r.len_qry[e.row], r.kmer, r.kspace, r.p_max, pr))
                    print_pair_line(o, r.ref.refs[e.col], r.qry.refs[e.row], r.comment, pr);
            });
        });
    vector<mg_result> res;
    for (Blocks b(0, r.nq, kDistFilteredPairs, r.nref); b.next();) {
        if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *n) {
                return mg_compare_rect_results_sharded_host(r.gpu.comm, r.dr.get(), r.dq.get(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, n); }))
            return 1;
        dist_emit_results(r, res);
    }
    return 0;
}

// -H: the spectrum of the pairs that pass -d and -v (one device: the first of those selected)
int dist_spectrum(DistRun &r)
{
    Spectrum sp;
    const bool filtered = r.d_max < 1.0 || r.p_max < 1.0;
    const uint64_t s = std::min(r.ref.p.sketch_size, r.qry.p.sketch_size);
    auto clamped = [&](const Ref &x) { return std::min<uint64_t>(x.hashes.size(), s); };
    vector<mg_spectrum_bin> bins;
    vector<mg_result> res;
    vector<mg_edge> edges;
    std::map<uint64_t, uint64_t> href;
    for (const Ref &x : r.ref.refs) href[clamped(x)]++;
    for (Blocks b(0, r.nq, kDistFilteredPairs, r.nref); b.next();) {
        if (!host_finish_wanted()) {
            if (!fetch_list(r.gpu, bins, [&](mg_spectrum_bin *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_rect_spectrum_host(r.gpu.ctx, r.tr, r.tq, b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, n); }))
                return 1;
            for (const mg_spectrum_bin &x : bins) sp.add(x.numer, x.denom, x.count);
        } else if (filtered) {
            if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_rect_results_host(r.gpu.ctx, r.tr, r.tq, b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, n); }))
                return 1;
            for (const mg_result &e : res) sp.add(e.numer, e.denom);
        } else {
            if (!fetch_list(r.gpu, edges, [&](mg_edge *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_rect_sparse_host(r.gpu.ctx, r.tr, r.tq, b.r0, b.r1, o, cap, n); }))
                return 1;
            for (uint64_t q = b.r0; q < b.r1; q++) sp.add_rule(s, clamped(r.qry.refs[q]), href);
            for (const mg_edge &e : edges) {
                sp.unlist(s, clamped(r.qry.refs[e.row]), clamped(r.ref.refs[e.col]));
                sp.add(e.numer, e.denom);
            }
        }
    }
    sp.print(r.out, r.kmer);
    return 0;
}

// Every pair: lines, or with -t one row of cells per query (writeOutput, CommandDistance.cpp:247-304)
int dist_full(DistRun &r)
{
    // -t without a p-value filter prints distances only: they come from one table per run
    // (a distance depends on numer / denom alone) and no p-value is evaluated
    DistText dtxt;
    const uint64_t s_tab = std::min(r.ref.p.sketch_size, r.qry.p.sketch_size);
    if (r.table && r.p_max >= 1.0 && s_tab <= (1u << 20) && !getenv("MASH_AMD_FULL_FINISH")) dtxt.build(s_tab, r.kmer, r.d_max);
    for (Blocks b(0, r.nq, kDistFullPairs, r.nref); b.next();) {
        const uint64_t q0 = b.r0;
        if (dtxt.on() || host_finish_wanted()) {
            if (dist_counts(r, b, !dtxt.on())) return 1;
        } else {
            // compare + distance + p-value + filters on the device, finished records back
            r.pairs.resize(b.npairs);
            if (mg_compare_rect_pairs_sharded_host(r.gpu.comm, r.dr.get(), r.dq.get(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.pairs.data()) != MG_OK)
                return report_error(r.gpu);
        }
        if (dtxt.on())
            emit_rows(r.out, b.r0, b.r1, [&](uint64_t) { return r.nref; }, [&](FastOut &o, uint64_t q, unsigned) {
                o << r.qry.refs[q].name;
                for (uint64_t x = 0; x < r.nref; x++) {
                    const mg_counts &c = r.counts[(q - q0) * r.nref + x];
                    dtxt.cell(o, c.numer, c.denom);
                    o.room();
                }
                o.eol();
            });
        else
            emit_rows(r.out, b.r0, b.r1, [&](uint64_t) { return r.nref; }, [&](FastOut &o, uint64_t q, unsigned) {
                if (r.table) o << r.qry.refs[q].name;
                for (uint64_t x = 0; x < r.nref; x++) {
                    const mg_pair &pr = r.pairs[(q - q0) * r.nref + x];
                    if (r.table) { o << '\t'; if (pr.pass) o << pr.distance; o.room(); }
                    else if (pr.pass) print_pair_line(o, r.ref.refs[x], r.qry.refs[q], r.comment, pr);
                }
                if (r.table) o.eol();
            });
    }
    return 0;
}

// What `dist` and `within` do with their first argument before a device is opened: a .msh reference refuses the options it
// fixes itself -- `fatal` end the run, `message_only` print the same message and the run goes on --, anything else is
// announced as being sketched.  Non-zero: refused.
int reference_announce(const Cmd &c, const string &file_ref, bool is_sketch, std::initializer_list<const char *> fatal,
                       std::initializer_list<const char *> message_only)
{
    if (!is_sketch) {
        cerr << "Sketching " << file_ref << " (provide sketch file made with \"mash sketch\" to skip)...";
        return 0;
    }
    auto refuse = [&](const char *o) {
        if (c.o(o).active) cerr << "ERROR: The option -" << c.o(o).id << " cannot be used when a sketch is provided; it is inherited from the sketch." << endl;
        return c.o(o).active;
    };
    for (const char *o : fatal) if (refuse(o)) return 1;
    for (const char *o : message_only) refuse(o);
    return 0;
}

// the parameters the queries are sketched with come from a .msh reference (CommandDistance.cpp:130-140, CommandContain.cpp:95-106)
void inherit_from_reference(Params &p, const SketchSet &ref)
{
    p.sketch_size = ref.p.sketch_size;
    p.kmer = ref.p.kmer;
    p.noncanonical = ref.p.noncanonical;
    p.preserve_case = ref.p.preserve_case;
    p.seed = ref.p.seed;
    set_alphabet(p, ref.p.alphabet);
}

int cmd_dist(int argc, const char **argv)
{
    Cmd c;
    c.name = "dist";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    c.add("table", Opt::Boolean, "t");
    c.add("pvalue", Opt::Number, "v", "1.0", 0., 1.);
    c.add("distance", Opt::Number, "d", "1.0", 0., 1.);
    c.add("comment", Opt::Boolean, "C");
    c.add("nearest", Opt::Integer, "N", "", 1, (float)MG_TOPK_MAX);          // (not in the reference: its user pipes through sort | head)
    c.add("spectrum", Opt::Boolean, "H");                                    // (not in the reference: ... | cut -f3,5 | sort | uniq -c)
    c.use_sketch_options();
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() < 2 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash dist [options] <reference> <query> [<query>] ...\n\n"
                "Output fields: [reference-ID, query-ID, distance, p-value, shared-hashes].\n"
                "Options: -l -t -v <max p> -d <max dist> -C -N <int> -H and the sketch options of `mash sketch`.\n"
                "  -N <int>  Per query at most <int> lines (1-" << MG_TOPK_MAX << "): its nearest references among those that pass -d and -v,\n"
                "            best first by shared-hashes as an exact fraction, equal fractions in reference order.\n"
                "  -H        The distance spectrum instead of the pairs: one line per distinct shared-hashes fraction among the pairs\n"
                "            that pass -d and -v, nearest first: [distance, shared-hashes, pairs, pairs at or below this distance].\n"
                "            Not with -t or -N.\n\n";
        return 0;
    }
    if (refuse_clashes(c, {{"nearest", "table"}, {"spectrum", "table"}, {"spectrum", "nearest"}})) return 1;
    const bool spectrum = c.o("spectrum").active;
    const uint32_t nearest = c.o("nearest").active ? (uint32_t)c.o("nearest").num : 0;
    const bool table = c.o("table").active, comment = c.o("comment").active;
    const double p_max = c.o("pvalue").num, d_max = c.o("distance").num;
    Params p;
    if (sketch_parameter_setup(p, c)) return 1;
    const string &file_ref = c.args[0];
    const bool is_sketch = has_suffix(file_ref, kSuffix);
    if (reference_announce(c, file_ref, is_sketch, {"kmer", "noncanonical", "protein", "alphabet"}, {})) return 1;
    Gpu gpu;
    SketchSet ref;
    init_from_files(gpu, ref, {file_ref}, p, is_sketch ? 1 : 0);
    KmerWarning w;
    if (is_sketch) {
        if (c.o("sketchSize").active && p.reads && p.sketch_size != ref.p.sketch_size) {        // CommandDistance.cpp:121-128
            cerr << "ERROR: The sketch size must match the reference when using a bloom filter (leave this option out to inherit from the reference sketch)." << endl;
            return 1;
        }
        inherit_from_reference(p, ref);
    } else {
        w = scan_kmer_warning(ref);
        cerr << "done.\n";
    }
    if (table) {
        cout << "#query";
        for (const Ref &r : ref.refs) cout << '\t' << r.name;
        cout << endl;
    }
    SketchSet qry;
    init_from_files(gpu, qry, input_files(c, 1), p, 0, true);
    const uint64_t nref = ref.refs.size(), nq = qry.refs.size();
    if (nref == 0 || nq == 0) return 0;
    // several GPUs: the larger side is cut into row blocks; references larger than the queries
    // are then not even replicated (the host-tail test paths address device 0's table as a whole)
    const bool ref_by_rows = mg_comm_size(gpu.comm) > 1 && nref > nq && !host_finish_wanted() && !getenv("MASH_AMD_NO_FILTER") && !spectrum;
    DistRun run(gpu, ref, qry, table, comment, nearest, d_max, p_max, ref_by_rows);
    if (spectrum ? dist_spectrum(run) : nearest ? dist_nearest(run) : !table && edge_filter_wanted(d_max, p_max) ? dist_filtered(run) : dist_full(run)) return 1;
    return finish_run(ref, w, p.reads);
}

// ------------------------------------------------------------------------------- within
// `mash within` (CommandContain.cpp): per query and reference, how much of the query's sketch lies inside the reference's --
// score = common / j and error = 1 / sqrt(j) of containSketches (:231-263), printed where error <= -e (writeOutput, :179-203).
// The device returns the two integers (mg_within_rect_results_host: only the pairs that pass -e cross PCIe; with
// MASH_AMD_HOST_FINISH=1 every pair's, filtered here); both doubles are formed here.
const uint64_t kWithinFullPairs = 1ull << 26;       // MASH_AMD_HOST_FINISH=1: 512 MiB of mg_counts per block

inline void print_within_line(FastOut &out, const Ref &ref, const Ref &qry, uint32_t common, uint32_t j)
{
    out << double(common) / j << '\t' << 1. / sqrt(j) << '\t' << ref.name << '\t' << qry.name;
    out.eol();
}

int cmd_within(int argc, const char **argv)
{
    Cmd c;
    c.name = "within";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    c.add("errorThreshold", Opt::Number, "e", "0.05");
    c.use_sketch_options();
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() < 2 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash within [options] <reference> <query> [<query>] ...\n\n"
                "Estimate the containment of each query file (or sequence with -i) in the reference: the number of\n"
                "intersecting min-hashes divided by the query set size.\n"
                "Output fields: [score, error-bound, reference-ID, query-ID].\n"
                "Options: -l -e <max error> and the sketch options of `mash sketch`.\n"
                "  -e <num>  Error bound threshold for reporting scores values. [0.05]\n\n";
        return 0;
    }
    // the threshold reaches writeOutput as a float (CommandContain.cpp:167, :179) and is compared as a double (:188)
    const double e_max = (double)c.o("errorThreshold").num;
    Params p;
    if (sketch_parameter_setup(p, c)) return 1;
    const string &file_ref = c.args[0];
    const bool is_sketch = has_suffix(file_ref, kSuffix);
    // (-a and -z print the refusal and the run goes on: CommandContain.cpp:73-81 has no `return 1`)
    if (reference_announce(c, file_ref, is_sketch, {"kmer", "noncanonical"}, {"protein", "alphabet"})) return 1;
    Gpu gpu;
    SketchSet ref;
    init_from_files(gpu, ref, {file_ref}, p, is_sketch ? 1 : 0);
    if (is_sketch) inherit_from_reference(p, ref);
    else cerr << "done.\n";
    SketchSet qry;
    init_from_files(gpu, qry, input_files(c, 1), p, 0, true, nullptr, true);     // (a smaller sketch size is accepted, Sketch.cpp:150)
    const uint64_t nref = ref.refs.size(), nq = qry.refs.size();
    if (nref == 0 || nq == 0) return 0;
    // the rows' own hash counts decide, so each table is as wide as its longest row
    uint64_t s_ref = 1, s_qry = 1;
    for (const Ref &r : ref.refs) s_ref = std::max<uint64_t>(s_ref, r.hashes.size());
    for (const Ref &r : qry.refs) s_qry = std::max<uint64_t>(s_qry, r.hashes.size());
    DTable dr(upload_all(gpu, ref, s_ref)), dq(upload_all(gpu, qry, s_qry));
    const mg_table *tr = mg_dtable_local(dr.get(), 0), *tq = mg_dtable_local(dq.get(), 0);
    FastOut out;
    if (host_finish_wanted()) {
        vector<mg_counts> counts;
        for (Blocks b(0, nq, kWithinFullPairs, nref); b.next();) {
            counts.resize(b.npairs);
            if (mg_within_rect_host(gpu.ctx, tr, tq, b.r0, b.r1, counts.data()) != MG_OK) return report_error(gpu);
            const uint64_t q0 = b.r0;
            emit_rows(out, b.r0, b.r1, [&](uint64_t) { return nref; }, [&](FastOut &o, uint64_t q, unsigned) {
                for (uint64_t x = 0; x < nref; x++) {
                    const mg_counts &k = counts[(q - q0) * nref + x];
                    if (k.denom && 1. / sqrt(k.denom) <= e_max) print_within_line(o, ref.refs[x], qry.refs[q], k.numer, k.denom);
                }
            });
        }
        return 0;
    }
    vector<mg_edge> res;
    for (Blocks b(0, nq, kDistFilteredPairs, nref); b.next();) {
        if (!fetch_list(gpu, res, [&](mg_edge *o, uint64_t cap, uint64_t *n) {
                return mg_within_rect_results_host(gpu.ctx, tr, tq, b.r0, b.r1, e_max, o, cap, n); }))
            return 1;
        emit_rows(out, 0, res.size(), [](uint64_t) { return 1; }, [&](FastOut &o, uint64_t x, unsigned) {
            const mg_edge &k = res[x];
            print_within_line(o, ref.refs[k.col], qry.refs[k.row], k.numer, k.denom);
        });
    }
    return 0;
}

// ------------------------------------------------------------------------------- triangle
// Budgets of a block of rows (MASH_AMD_BLOCK_PAIRS lowers them; kTriFilteredPairs stands with tri_edge_blocks):
const uint64_t kTriDensePairs = 1ull << 24;         // the whole block comes back: 128 MiB of mg_counts, 512 MiB of mg_pair
const uint64_t kTriSparsePairs = 1ull << 26;        // only the pairs that share a hash come back: at most an eighth of these
const uint64_t kTriNearestRecords = 1ull << 24;     // -N: `keep` records per row, 512 MiB of mg_result per block

struct TriRun {
    Gpu &gpu;
    const SketchSet &set;
    const bool comment, edge;
    const uint32_t nearest;
    const double d_max, p_max, kspace;
    const int kmer;
    const uint64_t n;
    vector<uint64_t> lengths;
    DTable dt;
    mg_table *t;                              // device 0's replica: what the calls on one context address
    DistText dtxt;                            // on: the Phylip rows are the lean ones (distances from the table,
    PeakPValue peak;                          //     p-values only where they can raise the peak)
    vector<mg_counts> counts;                 // (these keep their capacity over the blocks)
    vector<mg_pair> pairs;
    StageClock clk;                           // (starts when the table is on the devices)
    FastOut out;
    TriRun(Gpu &g, const SketchSet &s, bool comment_, bool edge_, uint32_t nearest_, double d_max_, double p_max_)
        : gpu(g), set(s), comment(comment_), edge(edge_), nearest(nearest_), d_max(d_max_), p_max(p_max_), kspace(s.kmer_space()), kmer(s.p.kmer),
          n(s.refs.size()), dt(upload_all(g, s, s.p.sketch_size, &lengths)), t(mg_dtable_local(dt.get(), 0))
    {
        if (edge || s.p.sketch_size > (1u << 20) || getenv("MASH_AMD_FULL_FINISH")) return;          // (env: the plain path, for tests)
        dtxt.build(s.p.sketch_size, kmer);
        peak.use_bound(lengths, s.p.sketch_size, kspace);
    }
    const string &label(uint64_t i) const { return comment ? set.refs[i].comment : set.refs[i].name; }
};

void tri_emit_results(TriRun &r, const vector<mg_result> &res)
{
    emit_rows(r.out, 0, res.size(), [](uint64_t) { return 1; }, [&](FastOut &o, uint64_t x, unsigned) {
        const mg_result &e = res[x];
        print_edge_line(o, r.label(e.row), r.label(e.col), e.numer, e.denom, e.distance, e.p_value);
    });
}

// -N: per sketch its nearest neighbours, ranked and cut on the device (mg_compare_tri_topk_host; one device: the first of
// those selected): N records per sketch cross PCIe.
int tri_nearest(TriRun &r, uint64_t keep)
{
    vector<mg_result> res;
    if (!host_finish_wanted()) {
        for (Blocks b(0, r.n, kTriNearestRecords, keep); b.next();) {
            if (res.size() < b.npairs) res.resize(b.npairs);                            // the largest possible answer: one call
            if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *cnt) {
                    return mg_compare_tri_topk_host(r.gpu.ctx, r.t, b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.nearest, o, cap, cnt); }))
                return 1;
            tri_emit_results(r, res);
        }
        return 0;
    }
    // MASH_AMD_HOST_FINISH=1: the triangle of counts, the host tail, both rows of a passing pair note it, and the same
    // selection here
    vector<vector<mg_result>> rows(r.n);                        // a row's passing pairs as {row, neighbour, ...}
    for (Blocks b(1, r.n, kTriDensePairs); b.next();) {
        r.counts.resize(b.npairs);
        r.pairs.resize(b.npairs);
        if (mg_compare_tri_sharded_host(r.gpu.comm, r.dt.get(), b.r0, b.r1, r.counts.data()) != MG_OK) return report_error(r.gpu);
        mg_finish_tri_host(r.counts.data(), r.lengths.data(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.pairs.data());
        uint64_t idx = 0;
        for (uint64_t i = b.r0; i < b.r1; i++)
            for (uint64_t j = 0; j < i; j++, idx++) {
                const mg_pair &a = r.pairs[idx];
                if (!a.pass) continue;
                rows[i].push_back(mg_result{(uint32_t)i, (uint32_t)j, a.numer, a.denom, a.distance, a.p_value});
                rows[j].push_back(mg_result{(uint32_t)j, (uint32_t)i, a.numer, a.denom, a.distance, a.p_value});
            }
    }
    for (vector<mg_result> &row : rows) select_nearest(row, keep, res);
    tri_emit_results(r, res);
    return 0;
}

// -E with -d / -v: the surviving pairs as finished records
int tri_filtered(TriRun &r)
{
    if (host_finish_wanted())
        // MASH_AMD_HOST_FINISH=1: the pairs within -d from device 0's replica, p-values and the -v filter here
        return tri_edge_blocks(r.gpu, r.t, r.n, r.kmer, r.d_max, [&](const vector<mg_edge> &edges) {
            r.clk.lap("compare+filter+copy");
            emit_rows(r.out, 0, edges.size(), [](uint64_t) { return 1; }, [&](FastOut &o, uint64_t x, unsigned) {
                const mg_edge &e = edges[x];
                mg_pair pr;
                if (finish_edge(e, r.lengths[e.row], r.lengths[e.col], r.kmer, r.kspace, r.p_max, pr))
                    print_edge_line(o, r.label(e.row), r.label(e.col), pr.numer, pr.denom, pr.distance, pr.p_value);
            });
            r.clk.lap("finish+format+write");
        });
    vector<mg_result> res;
    for (Blocks b(1, r.n, kTriFilteredPairs); b.next();) {
        if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *cnt) {
                return mg_compare_tri_results_sharded_host(r.gpu.comm, r.dt.get(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, cnt); }))
            return 1;
        r.clk.lap("compare+finish+filter+copy");
        tri_emit_results(r, res);
        r.clk.lap("format+write");
    }
    return 0;
}

// The Phylip matrix from the SPARSE result (mg_compare_tri_sparse_host): a pair that shares no hash is {0, min(s, |A| + |B|)}
// -- distance 1, p-value 1 -- and in a collection nearly every pair is such a pair: what crosses PCIe and is looked at are
// the exceptions, a row's text is runs of "\t1" between them (CommandTriangle.cpp:159-198 writes the same cells).  One
// device; a block whose exceptions outnumber an eighth of its pairs (one species: every pair shares hashes) ends this route
// with r0 at its first row: tri_dense, which has the engines for that, takes the rest of the run.
int tri_sparse(TriRun &r, uint64_t &r0)
{
    if (!r.dtxt.on() || mg_comm_size(r.gpu.comm) != 1 || getenv("MASH_AMD_DENSE_MATRIX")) return 0;      // (env: dense from the start)
    const DistText &dtxt = r.dtxt;
    vector<mg_edge> exc;
    vector<uint64_t> exc_at;
    string ones;
    for (int k = 0; k < 4096; k++) ones += "\t1";
    for (Blocks b(r0, r.n, kTriSparsePairs); b.next(); r0 = b.r1) {
        r.clk.lap("setup");
        const uint64_t cap = b.npairs / 8 + 4096, b0 = b.r0;
        if (exc.size() < cap) exc.resize(cap);
        uint64_t cnt = 0;
        const int rc = mg_compare_tri_sparse_host(r.gpu.ctx, r.t, b.r0, b.r1, exc.data(), cap, &cnt);
        if (rc == MG_ERR_NOMEM) return 0;
        if (rc != MG_OK) return report_error(r.gpu);
        r.clk.lap("compare+sparse result+copy");
        exc_at.assign(b.r1 - b0 + 1, cnt);                     // exceptions of row i: exc[exc_at[i - b0] .. exc_at[i - b0 + 1])
        for (uint64_t x = cnt; x-- > 0;) exc_at[exc[x].row - b0] = x;
        for (uint64_t i = b.r1 - b0; i-- > 0;) if (exc_at[i] > exc_at[i + 1]) exc_at[i] = exc_at[i + 1];
        r.peak.begin();
        emit_rows(r.out, b.r0, b.r1, [](uint64_t i) { return i / 16 + 64; }, [&](FastOut &o, uint64_t i, unsigned slot) {
            double pk = r.peak.slot[slot];
            o << r.label(i);
            const bool empty_row = r.set.refs[i].hashes.empty();
            auto defaults = [&](uint64_t c0, uint64_t c1) {       // columns [c0, c1) share nothing with row i
                if (c0 >= c1) return;
                if (pk < 1.0) pk = 1.0;                          // pValue(0, ...) = 1 (CommandDistance.cpp:431-434)
                if (!empty_row) {
                    for (uint64_t m = c1 - c0; m;) { const uint64_t k = std::min<uint64_t>(m, 4096); o.buf.append(ones, 0, 2 * k); m -= k; }
                } else {
                    // (two empty sketches: 0 / 0 union elements, common == denom: distance 0, CommandDistance.cpp:390-393)
                    for (uint64_t j = c0; j < c1; j++) o << (r.set.refs[j].hashes.empty() ? "\t0" : "\t1");
                }
                o.room();
            };
            uint64_t c = 0;
            for (uint64_t x = exc_at[i - b0]; x < exc_at[i - b0 + 1]; x++) {
                const mg_edge &e = exc[x];
                defaults(c, e.col);
                dtxt.cell(o, e.numer, e.denom);
                r.peak.note(pk, e.numer, e.denom, r.lengths[i], r.lengths[e.col]);
                c = (uint64_t)e.col + 1;
            }
            defaults(c, i);
            r.peak.slot[slot] = pk;
            o.eol();
        });
        r.peak.merge();
        r.clk.lap("format+write");
    }
    return 0;
}

// Rows [r0, n) from the whole matrix of counts: the lean Phylip rows (dtxt: distances from the table, p-values only where
// they can raise the peak), or every pair finished -- on the device, with MASH_AMD_HOST_FINISH=1 on the host -- for the
// plain Phylip rows (MASH_AMD_FULL_FINISH=1) and the unfiltered edge list (writeOutput, CommandTriangle.cpp:159-198)
int tri_dense(TriRun &r, uint64_t r0)
{
    const DistText &dtxt = r.dtxt;
    const bool lean = dtxt.on(), edge = r.edge;
    for (Blocks b(r0, r.n, kTriDensePairs); b.next();) {
        const bool dev_finish = !lean && !host_finish_wanted();
        if (!dev_finish) r.counts.resize(b.npairs);
        if (!lean) r.pairs.resize(b.npairs);
        r.clk.lap("setup");
        if (dev_finish) {
            if (mg_compare_tri_pairs_sharded_host(r.gpu.comm, r.dt.get(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.pairs.data()) != MG_OK)
                return report_error(r.gpu);
            r.clk.lap("compare+finish+copy");
        } else {
            if (mg_compare_tri_sharded_host(r.gpu.comm, r.dt.get(), b.r0, b.r1, r.counts.data()) != MG_OK) return report_error(r.gpu);
            r.clk.lap("compare+copy");
            if (!lean) mg_finish_tri_host(r.counts.data(), r.lengths.data(), b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, r.pairs.data());
            r.clk.lap("finish");
        }
        const uint64_t base = b.r0 * (b.r0 - 1) / 2;
        r.peak.begin();
        if (lean) {
            emit_rows(r.out, b.r0, b.r1, [](uint64_t i) { return i; }, [&](FastOut &o, uint64_t i, unsigned slot) {
                uint64_t idx = i * (i - 1) / 2 - base;
                double pk = r.peak.slot[slot];
                o << r.label(i);
                for (uint64_t j = 0; j < i; j++, idx++) {
                    const mg_counts &c = r.counts[idx];
                    dtxt.cell(o, c.numer, c.denom);
                    o.room();
                    r.peak.note(pk, c.numer, c.denom, r.lengths[i], r.lengths[j]);
                }
                r.peak.slot[slot] = pk;
                o.eol();
            });
        } else {
            emit_rows(r.out, b.r0, b.r1, [](uint64_t i) { return i; }, [&](FastOut &o, uint64_t i, unsigned slot) {
                uint64_t idx = i * (i - 1) / 2 - base;
                double pk = r.peak.slot[slot];
                if (!edge) o << r.label(i);
                for (uint64_t j = 0; j < i; j++, idx++) {
                    const mg_pair &pr = r.pairs[idx];
                    if (edge) {
                        if (pr.pass) print_edge_line(o, r.label(i), r.label(j), pr.numer, pr.denom, pr.distance, pr.p_value);
                    } else {
                        o << '\t' << pr.distance;
                        o.room();
                    }
                    if (pr.p_value > pk) pk = pr.p_value;
                }
                r.peak.slot[slot] = pk;
                if (!edge) o.eol();
            });
        }
        r.peak.merge();
        r.clk.lap("format+write");
    }
    return 0;
}

// -H: the spectrum of the pairs that pass -d and -v (one device: the first of those selected)
int tri_spectrum(TriRun &r)
{
    Spectrum sp;
    const bool filtered = r.d_max < 1.0 || r.p_max < 1.0;
    const uint64_t s = r.set.p.sketch_size;
    auto clamped = [&](uint64_t i) { return std::min<uint64_t>(r.set.refs[i].hashes.size(), s); };
    vector<mg_spectrum_bin> bins;
    vector<mg_result> res;
    vector<mg_edge> edges;
    std::map<uint64_t, uint64_t> below;                           // the clamped hash counts of the rows ahead of the one at hand
    if (r.n) below[clamped(0)]++;
    for (Blocks b(1, r.n, kTriFilteredPairs); b.next();) {
        if (!host_finish_wanted()) {
            if (!fetch_list(r.gpu, bins, [&](mg_spectrum_bin *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_tri_spectrum_host(r.gpu.ctx, r.t, b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, n); }))
                return 1;
            for (const mg_spectrum_bin &x : bins) sp.add(x.numer, x.denom, x.count);
        } else if (filtered) {
            if (!fetch_list(r.gpu, res, [&](mg_result *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_tri_results_host(r.gpu.ctx, r.t, b.r0, b.r1, r.kmer, r.kspace, r.d_max, r.p_max, o, cap, n); }))
                return 1;
            for (const mg_result &e : res) sp.add(e.numer, e.denom);
        } else {
            if (!fetch_list(r.gpu, edges, [&](mg_edge *o, uint64_t cap, uint64_t *n) {
                    return mg_compare_tri_sparse_host(r.gpu.ctx, r.t, b.r0, b.r1, o, cap, n); }))
                return 1;
            for (uint64_t i = b.r0; i < b.r1; i++) {
                sp.add_rule(s, clamped(i), below);
                below[clamped(i)]++;
            }
            for (const mg_edge &e : edges) {
                sp.unlist(s, clamped(e.row), clamped(e.col));
                sp.add(e.numer, e.denom);
            }
        }
    }
    sp.print(r.out, r.kmer);
    return 0;
}

int cmd_triangle(int argc, const char **argv)
{
    Cmd c;
    c.name = "triangle";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    c.add("comment", Opt::Boolean, "C");
    c.add("edge", Opt::Boolean, "E");
    c.add("pvalue", Opt::Number, "v", "1.0", 0., 1.);
    c.add("distance", Opt::Number, "d", "1.0", 0., 1.);
    c.add("nearest", Opt::Integer, "N", "", 1, (float)MG_TOPK_MAX);          // (not in the reference)
    c.add("spectrum", Opt::Boolean, "H");                                    // (not in the reference)
    c.use_sketch_options();
    if (c.parse(argc, argv)) return 1;
    if (c.args.empty() || c.o("help").active) {
        cout << "\nUsage:\n\n  mash triangle [options] <seq1> [<seq2>] ...\n\n"
                "Lower-triangular distance matrix in relaxed Phylip format (or -E edge list).\n"
                "Options: -l -C -E -v <max p> -d <max dist> -N <int> -H and the sketch options of `mash sketch`.\n"
                "  -N <int>  Per sketch, in input order, at most <int> edge-list lines (1-" << MG_TOPK_MAX << "): its nearest neighbours among the other\n"
                "            sketches that pass -d and -v, best first by shared-hashes as an exact fraction, equal fractions in input\n"
                "            order.  Implies -E; a pair can appear under both its sketches.\n"
                "  -H        The distance spectrum instead of the matrix: one line per distinct shared-hashes fraction among the pairs\n"
                "            that pass -d and -v, nearest first: [distance, shared-hashes, pairs, pairs at or below this distance] --\n"
                "            the last field is the number of lines -E -d <distance> would print.  Not with -E or -N.\n\n";
        return 0;
    }
    if (refuse_clashes(c, {{"spectrum", "edge"}, {"spectrum", "nearest"}})) return 1;
    const bool spectrum = c.o("spectrum").active;
    const uint32_t nearest = c.o("nearest").active ? (uint32_t)c.o("nearest").num : 0;
    const bool comment = c.o("comment").active;
    bool edge = c.o("edge").active;
    const double p_max = c.o("pvalue").num, d_max = c.o("distance").num;
    if (c.o("pvalue").active || c.o("distance").active || nearest || spectrum) edge = true;
    Params p;
    if (sketch_parameter_setup(p, c)) return 1;
    if (c.args.size() == 1 && !c.o("list").active) p.concatenated = false;   // CommandTriangle.cpp:74-77
    Gpu gpu;
    SketchSet set;
    init_from_files(gpu, set, input_files(c), p, 1);
    const KmerWarning w = scan_kmer_warning(set);
    const uint64_t n = set.refs.size();
    if (n == 0) return 0;
    if (!edge) {
        cout << '\t' << n << endl;
        cout << (comment ? set.refs[0].comment : set.refs[0].name) << endl;
    }
    TriRun run(gpu, set, comment, edge, nearest, d_max, p_max);
    const uint64_t keep = std::min<uint64_t>(nearest, n - 1);
    if (nearest && !keep) return 0;                              // one sketch: no neighbour to rank
    uint64_t r0 = 1;                                             // the row at which the sparse route hands over to the dense one
    if (spectrum ? tri_spectrum(run) : nearest ? tri_nearest(run, keep) : edge && edge_filter_wanted(d_max, p_max) ? tri_filtered(run) : tri_sparse(run, r0) || tri_dense(run, r0)) return 1;
    run.dt.reset();                                              // (inside the "teardown" lap, as the later lines)
    if (!edge) cerr << "Max p-value: " << run.peak.peak << endl;
    return finish_run(set, w, p.reads);
}

// `mash cluster`: single-linkage clusters of the pairs `mash triangle -E -d -v` would print (the reference has no such command;
// include/mashgpu.h: mg_cluster_tri_host).  One line per sketch in input order: cluster number (from 1, in order of the
// clusters' first members), cluster size, name.  The clusters are found on the device and one label per sketch comes back.
// -R: greedy representative clusters of the same pairs instead (mg_cluster_tri_greedy_host): walking the sketches in input
// order, a sketch opens a cluster iff no earlier representative is within the threshold, else it joins the first one that is.
// Lines and numbering are the same (the label is the representative).
// -B: -R's representatives, every other sketch under its NEAREST one (mg_cluster_tri_nearest_host): the representative, earlier or
// later in the input, with which it shares the larger fraction of hashes, exactly (mg::forest_before); a fourth field names it.
// -M: the single-linkage clusters, each line with a fourth field naming the cluster's MEDOID (mg_cluster_tri_medoid_host): the member
// whose edges' weights floor(numer * 2^32 / max(denom, 1)) sum to the most, equal sums to the earlier member.  Numbers, sizes and
// the first three fields are those of the run without -M.
// -T: the minimum spanning forest of the same pairs instead (mg_cluster_tri_forest_host): one `triangle -E` line per forest edge,
// best first, not cluster lines.
// -L: complete-linkage clusters of the same pairs instead (mg_cluster_tri_complete_host): every two members of a cluster are an
// edge; links merge best first by the exact fraction of their worst pair.  Lines and numbering are those of the plain run.
// -D <m>: density clusters of the same pairs instead (mg_cluster_tri_density_host): a sketch with at least m edges is a core, cores
// cluster over the edges between them, any other sketch with an edge to a core is a border under its nearest core, the rest is noise.
// Lines get two more fields, the role and the number of edges; with -D 1 the first three fields are those of the plain run.
// -A <earlier output>: the clusters of the first L inputs are read from an earlier run's stdout and only the pairs that touch a
// later input are compared (cluster_extend below; include/mashgpu.h: mg_cluster_extend_host).  With plain and with -R only.
// MASH_AMD_HOST_FINISH=1 is the host route, which the tests judge the device route by: the pairs within -d come from the host calls
// of `triangle -E -d` and `dist -d` (tri_edge_blocks, rect_edge_blocks), and what follows is done here, once for every form
// (cluster_on_host: Sets, greedy_walk, nearest_pick, medoid_pick; -T: Kruskal over the same Sets; -L: complete_walk; -D: density_walk).

enum ClusterMode { kSingle, kGreedy, kNearest, kMedoid, kForest, kComplete, kDensity };      // plain, -R, -B (with or without -R), -M, -T, -L, -D; -A is a flag beside it

// The lap of a form's clustering (MASH_AMD_TIMING=1) on the device and on the host route: kClusterLaps[mode][with -A]
const struct { const char *device, *host; } kClusterLaps[7][2] = {
    {{"compare+mark+union+label+copy", "compare+filter+copy+union"},
     {"seed+compare+mark+union (new x old, new x new)+label+copy", "compare+filter+copy (new x old, new x new)+union"}},
    {{"compare+mark+append+rounds+assign+copy", "compare+filter+copy+walk"},
     {"compare+mark+append (new x representatives, new x new)+rounds+assign+copy", "compare+filter+copy (new x representatives, new x new)+walk"}},
    {{"compare+mark+append+rounds+nearest+copy", "compare+filter+copy+walk+nearest"}},
    {{"compare+mark+union+score+label+pick+copy", "compare+filter+copy+union+score+pick"}},
    {{"compare+mark+append+rounds+sort+finish+copy", "compare+filter+copy+sort+kruskal"}},
    {{"compare+mark+append+index+rounds+label+copy", "compare+filter+copy+walk"}},
    {{"compare+mark+append+degree+union+border+label+copy", "compare+filter+copy+degree+union+border"}},
};

// Union-find in place over a vector of labels: a set's root is its smallest member, so the first input of a cluster names it
struct Sets {
    vector<uint32_t> &up;
    uint32_t find(uint32_t x) { while (up[x] != x) { up[x] = up[up[x]]; x = up[x]; } return x; }
    bool unite(uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a != b) up[std::max(a, b)] = std::min(a, b); return a != b; }      // false: one set already
};

// -R: the walk over the inputs from `first` on, in input order; smaller[i - first] holds the neighbours of i with a smaller index.
// lab[j] == j says that j, decided before i, is a representative: i joins the first such neighbour and stays its own without one.
void greedy_walk(vector<uint32_t> &lab, uint64_t first, const vector<vector<uint32_t>> &smaller)
{
    for (uint64_t i = first; i < lab.size(); i++)
        for (const uint32_t j : smaller[i - first])
            if (lab[j] == j && (lab[i] == i || j < lab[i])) lab[i] = j;
}

// -B: the walk has named the representatives; a member now takes the best of ALL its edges to one, either end of the pair:
// mg::forest_before with the representative in the row pair's place (equal fractions: the smaller one)
void nearest_pick(vector<uint32_t> &lab, const vector<mg_edge> &edges)
{
    const uint64_t n = lab.size();
    vector<uint8_t> is_rep(n);
    vector<const mg_edge *> best(n, nullptr);
    for (uint64_t i = 0; i < n; i++) is_rep[i] = lab[i] == i;
    for (const mg_edge &e : edges) {
        if (is_rep[e.row] == is_rep[e.col]) continue;
        const uint32_t member = is_rep[e.row] ? e.col : e.row, r = is_rep[e.row] ? e.row : e.col;
        const mg_edge *b = best[member];
        if (!b || mg::forest_before(e.numer, e.denom, r, b->numer, b->denom, lab[member])) {
            best[member] = &e;
            lab[member] = r;
        }
    }
}

// -M: per cluster the largest score, met first at its smallest row: the walk is in index order and only a larger score moves it
void medoid_pick(const vector<uint32_t> &lab, const vector<uint64_t> &score, vector<uint32_t> &med)
{
    const uint64_t n = lab.size();
    vector<uint32_t> top(n);
    for (uint64_t i = 0; i < n; i++) top[i] = (uint32_t)i;
    for (uint64_t i = 0; i < n; i++)
        if (score[i] > score[top[lab[i]]]) top[lab[i]] = (uint32_t)i;
    for (uint64_t i = 0; i < n; i++) med[i] = top[lab[i]];
}

// -L: the sequential walk of the definition (include/mashgpu.h: mg_cluster_tri_complete_host).  links[a][b], for cluster ids a and b
// either way round, holds the counts of the worst edge between the two clusters, present iff every pair between them is an edge;
// `order` holds every link once, best first (mg::forest_before over {larger id, smaller id}).  The first link is merged: the
// survivor's links are those BOTH clusters had, each with the worse of the two weights.
void complete_walk(vector<uint32_t> &lab, const vector<mg_edge> &edges)
{
    struct Weight { uint32_t numer, denom; };
    struct Link { uint32_t numer, denom; uint64_t rc; };
    auto before = [](const Link &a, const Link &b) { return mg::forest_before(a.numer, a.denom, a.rc, b.numer, b.denom, b.rc); };
    auto link_of = [](uint32_t a, uint32_t b, const Weight &w) { return Link{w.numer, w.denom, mg::forest_rc(std::max(a, b), std::min(a, b))}; };
    vector<std::map<uint32_t, Weight>> links(lab.size());
    std::set<Link, decltype(before)> order(before);
    for (const mg_edge &e : edges) {
        const Weight w{e.numer, e.denom};
        links[e.row][e.col] = links[e.col][e.row] = w;
        order.insert(link_of(e.row, e.col, w));
    }
    vector<uint32_t> up(lab.size());
    for (size_t i = 0; i < up.size(); i++) up[i] = (uint32_t)i;
    while (!order.empty()) {
        const Link first = *order.begin();
        const uint32_t gone = (uint32_t)(first.rc >> 32), stay = (uint32_t)first.rc;
        std::map<uint32_t, Weight> merged;
        for (const auto &[other, w] : links[gone]) {
            order.erase(link_of(gone, other, w));
            links[other].erase(gone);
            const auto at = links[stay].find(other);
            if (other == stay || at == links[stay].end()) continue;
            // the worse of the two: the smaller fraction (equal fractions: either, the key of the order is the same)
            merged[other] = mg::forest_before(w.numer, w.denom, 0, at->second.numer, at->second.denom, 0) ? at->second : w;
        }
        for (const auto &[other, w] : links[stay]) {
            if (other == gone) continue;
            order.erase(link_of(stay, other, w));
            links[other].erase(stay);
        }
        for (const auto &[other, w] : merged) {
            links[other][stay] = w;
            order.insert(link_of(stay, other, w));
        }
        links[gone].clear();
        links[stay] = std::move(merged);
        up[gone] = stay;
    }
    Sets sets{up};
    for (size_t i = 0; i < lab.size(); i++) lab[i] = sets.find((uint32_t)i);
}

// What a run finds: per input its label, the first member of its cluster (-R, -B: its representative), and with -M its cluster's
// medoid; or with -T the forest's records, best first; with -D (min_nb: its argument) per input the core it came in by and its edges
struct Clusters { vector<uint32_t> lab, med; vector<mg_result> forest; uint32_t min_nb = 0; vector<uint32_t> via, deg; };

// -D: the definition (include/mashgpu.h: mg_cluster_tri_density_host) over the kept edges: degrees, the cores united over the edges
// between two of them, a border under the best of its edges to a core (mg::forest_before with the core in the row pair's place),
// then every cluster named by its first member, borders included
void density_walk(Clusters &c, const vector<mg_edge> &edges)
{
    vector<uint32_t> &lab = c.lab, &via = c.via, &deg = c.deg;
    const uint64_t n = lab.size();
    std::fill(deg.begin(), deg.end(), 0u);
    for (const mg_edge &e : edges) { deg[e.row]++; deg[e.col]++; }
    auto core = [&](uint32_t i) { return deg[i] >= c.min_nb; };
    Sets sets{lab};
    vector<const mg_edge *> best(n, nullptr);
    for (uint64_t i = 0; i < n; i++) via[i] = (uint32_t)i;
    for (const mg_edge &e : edges) {
        if (core(e.row) && core(e.col)) sets.unite(e.row, e.col);
        if (core(e.row) == core(e.col)) continue;
        const uint32_t member = core(e.row) ? e.col : e.row, k = core(e.row) ? e.row : e.col;
        const mg_edge *b = best[member];
        if (!b || mg::forest_before(e.numer, e.denom, k, b->numer, b->denom, via[member])) {
            best[member] = &e;
            via[member] = k;
        }
    }
    vector<uint32_t> root(n), first(n, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < n; i++) root[i] = sets.find(via[i]);
    for (uint64_t i = 0; i < n; i++) first[root[i]] = std::min(first[root[i]], (uint32_t)i);
    for (uint64_t i = 0; i < n; i++) lab[i] = first[root[i]];
}

// The host route of every form, with and without -A, from the passing edges.  Inputs below `first` are decided already and lab
// holds their labels (-A: first == L; else 0).  passing_edges(take) calls take(edge, pair) for every edge that passes -d and -v,
// row and col being inputs, and returns non-zero after a reported error.  -T sorts them by the exact fraction and runs Kruskal.
template <class Source>
int cluster_on_host(ClusterMode mode, uint64_t first, Clusters &c, Source passing_edges)
{
    vector<uint32_t> &lab = c.lab;
    const uint64_t n = lab.size();
    const bool greedy = mode == kGreedy || mode == kNearest;
    for (uint64_t i = first; i < n; i++) lab[i] = (uint32_t)i;
    Sets sets{lab};
    vector<vector<uint32_t>> smaller(greedy ? n - first : 0);
    vector<mg_edge> kept;                                      // -B, -L, -D: every edge with its counts
    vector<uint64_t> score(mode == kMedoid ? n : 0);           // -M: per input the sum of its edges' weights
    vector<mg_result> all;                                     // -T: every edge as the record of its line
    if (passing_edges([&](const mg_edge &e, const mg_pair &pr) {
            if (mode == kForest) {
                all.push_back(mg_result{e.row, e.col, pr.numer, pr.denom, pr.distance, pr.p_value});
            } else if (mode == kComplete || mode == kDensity) {
                kept.push_back(e);
            } else if (greedy) {
                smaller[std::max(e.row, e.col) - first].push_back(std::min(e.row, e.col));
                if (mode == kNearest) kept.push_back(e);
            } else {
                sets.unite(e.row, e.col);
                if (mode == kMedoid) {
                    const uint64_t wt = mg::medoid_weight(e.numer, e.denom);
                    score[e.row] += wt;
                    score[e.col] += wt;
                }
            }
        }))
        return 1;
    if (mode == kForest) {
        std::sort(all.begin(), all.end(), [](const mg_result &a, const mg_result &b) {
            return mg::forest_before(a.numer, a.denom, mg::forest_rc(a.row, a.col), b.numer, b.denom, mg::forest_rc(b.row, b.col)); });
        for (const mg_result &e : all)
            if (sets.unite(e.row, e.col)) c.forest.push_back(e);
    } else if (mode == kComplete) {
        complete_walk(lab, kept);
    } else if (mode == kDensity) {
        density_walk(c, kept);
    } else if (greedy) {
        greedy_walk(lab, first, smaller);
        if (mode == kNearest) nearest_pick(lab, kept);
    } else {
        for (uint64_t i = 0; i < n; i++) lab[i] = sets.find((uint32_t)i);
        if (mode == kMedoid) medoid_pick(lab, score, c.med);
    }
    return 0;
}

// Every form without -A, on one table
int cluster_table(TriRun &r, ClusterMode mode, Clusters &c)
{
    if (host_finish_wanted()) {
        if (cluster_on_host(mode, 0, c, [&](auto take) {
                return tri_edge_blocks(r.gpu, r.t, r.n, r.kmer, r.d_max, [&](const vector<mg_edge> &edges) {
                    mg_pair pr;
                    for (const mg_edge &e : edges)
                        if (finish_edge(e, r.lengths[e.row], r.lengths[e.col], r.kmer, r.kspace, r.p_max, pr)) take(e, pr);
                });
            }))
            return 1;
        r.clk.lap(kClusterLaps[mode][0].host);
        return 0;
    }
    uint64_t count = 0, n_clusters = 0, n_edges = 0;
    int rc = MG_OK;
    switch (mode) {
    case kSingle: rc = mg_cluster_tri_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.lab.data(), &n_clusters, &n_edges); break;
    case kGreedy: rc = mg_cluster_tri_greedy_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.lab.data(), &n_clusters, &n_edges); break;
    case kNearest: rc = mg_cluster_tri_nearest_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.lab.data(), &n_clusters, &n_edges); break;
    case kMedoid: rc = mg_cluster_tri_medoid_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.lab.data(), c.med.data(), nullptr, &n_clusters, &n_edges); break;
    case kForest:
        c.forest.resize(r.n - 1);
        rc = mg_cluster_tri_forest_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.forest.data(), c.forest.size(), &count, nullptr, &n_clusters, &n_edges);
        break;
    case kComplete: rc = mg_cluster_tri_complete_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.lab.data(), &n_clusters, &n_edges); break;
    case kDensity:
        rc = mg_cluster_tri_density_host(r.gpu.ctx, r.t, r.kmer, r.kspace, r.d_max, r.p_max, c.min_nb, c.lab.data(), c.via.data(), c.deg.data(), &n_clusters, &n_edges);
        break;
    }
    if (rc != MG_OK) return report_error(r.gpu);
    c.forest.resize(count);
    r.clk.lap(kClusterLaps[mode][0].device);
    return 0;
}

// `mash cluster -A`: what an earlier run printed for the first L inputs -- per line its ID and its label, the first line that
// carries its cluster number (the cluster's first member, with -R its representative: a representative precedes its members)
struct Earlier {
    vector<string> id;
    vector<uint32_t> label;
};

// Reads the lines `<number>\t<size>\t<ID>` (the ID is everything behind the second tab; the size is not used).  false: an ERROR
// line has been printed.  Nothing here needs a device.
bool read_earlier(const string &path, Earlier &e)
{
    std::ifstream in(path);
    if (!in) {
        cerr << "ERROR: Could not open " << path << " for reading." << endl;
        return false;
    }
    std::map<uint64_t, uint32_t> first;      // cluster number -> the first line that carries it
    string line;
    while (std::getline(in, line)) {
        const uint64_t at = e.id.size() + 1;
        const size_t t1 = line.find('\t'), t2 = t1 == string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == string::npos) {
            cerr << "ERROR: Line " << at << " of " << path << " is not a line of `mash cluster` (number, size and ID between tabs)." << endl;
            return false;
        }
        uint64_t number = 0;
        bool good = t1 > 0 && t1 <= 18;
        for (size_t k = 0; good && k < t1; k++) {
            good = line[k] >= '0' && line[k] <= '9';
            number = number * 10 + (uint64_t)(line[k] - '0');
        }
        if (!good || number == 0) {
            cerr << "ERROR: Line " << at << " of " << path << " does not begin with a cluster number (a positive integer)." << endl;
            return false;
        }
        e.label.push_back(first.emplace(number, (uint32_t)e.id.size()).first->second);
        e.id.push_back(line.substr(t2 + 1));
    }
    if (!in.eof()) {                          // (a directory, a device that fails)
        cerr << "ERROR: Could not read " << path << "." << endl;
        return false;
    }
    return true;
}

// `mash cluster -A`: lab[i] for all n inputs from the earlier labels of the first L and the edges that touch a later input.  Plain:
// the first L sketches are one table, the rest a second one (mg_cluster_extend_host).  -R: only the earlier representatives are
// uploaded beside the new sketches -- edges to earlier members decide nothing -- and the indices are mapped back
// (mg_cluster_extend_greedy_host with ref_rep == NULL).  MASH_AMD_HOST_FINISH=1 takes the edges of the host calls of `dist -d` and
// `triangle -E -d` over the same two tables, as edges between inputs, to cluster_on_host.
int cluster_extend(Gpu &gpu, const SketchSet &set, const Earlier &old, ClusterMode mode, double d_max, double p_max, StageClock &clk, Clusters &c)
{
    vector<uint32_t> &lab = c.lab;
    const bool greedy = mode == kGreedy;
    const uint64_t n = set.refs.size(), L = old.id.size(), m = n - L;
    vector<uint32_t> ref_rows, qry_rows;     // the inputs behind the rows of the two tables
    for (uint64_t i = 0; i < L; i++)
        if (!greedy || old.label[i] == i) ref_rows.push_back((uint32_t)i);
    for (uint64_t i = L; i < n; i++) qry_rows.push_back((uint32_t)i);
    const uint64_t nref = ref_rows.size();
    auto input_of = [&](uint32_t x) { return x < nref ? ref_rows[x] : (uint32_t)(L + (x - nref)); };      // a row of ref + qry
    vector<uint64_t> len_ref, len_qry;
    DTable dr(upload_all(gpu, set, set.p.sketch_size, &len_ref, false, &ref_rows)), dq(upload_all(gpu, set, set.p.sketch_size, &len_qry, false, &qry_rows));
    mg_table *tr = mg_dtable_local(dr.get(), 0), *tq = mg_dtable_local(dq.get(), 0);      // (several devices selected: the first one's replicas)
    const double kspace = set.kmer_space();
    const int kmer = set.p.kmer;
    clk.lap("upload (earlier, new)");
    std::copy(old.label.begin(), old.label.end(), lab.begin());
    if (!host_finish_wanted()) {
        uint64_t n_clusters = 0, n_edges = 0;
        if (greedy) {
            vector<uint32_t> rep(std::max<uint64_t>(m, 1));
            if (mg_cluster_extend_greedy_host(gpu.ctx, tr, tq, nullptr, kmer, kspace, d_max, p_max, rep.data(), &n_clusters, &n_edges) != MG_OK)
                return report_error(gpu);
            for (uint64_t q = 0; q < m; q++) lab[L + q] = input_of(rep[q]);
        } else {
            if (mg_cluster_extend_host(gpu.ctx, tr, tq, old.label.data(), kmer, kspace, d_max, p_max, lab.data(), &n_clusters, &n_edges) != MG_OK)
                return report_error(gpu);
        }
        clk.lap(kClusterLaps[mode][1].device);
        return 0;
    }
    // new x earlier (with -R: x the earlier representatives), then new x new; the walk and the unions go on from the earlier labels
    if (cluster_on_host(mode, L, c, [&](auto take) {
            mg_pair pr;
            if (nref && rect_edge_blocks(gpu, tr, tq, nref, m, kmer, d_max, [&](const vector<mg_edge> &edges) {
                    for (const mg_edge &e : edges)
                        if (finish_edge(e, len_ref[e.col], len_qry[e.row], kmer, kspace, p_max, pr))
                            take(mg_edge{(uint32_t)(L + e.row), ref_rows[e.col], e.numer, e.denom}, pr);
                }))
                return 1;
            return tri_edge_blocks(gpu, tq, m, kmer, d_max, [&](const vector<mg_edge> &edges) {
                for (const mg_edge &e : edges)
                    if (finish_edge(e, len_qry[e.row], len_qry[e.col], kmer, kspace, p_max, pr))
                        take(mg_edge{(uint32_t)(L + e.row), (uint32_t)(L + e.col), e.numer, e.denom}, pr);
            });
        }))
        return 1;
    clk.lap(kClusterLaps[mode][1].host);
    return 0;
}

int cmd_cluster(int argc, const char **argv)
{
    Cmd c;
    c.name = "cluster";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    c.add("comment", Opt::Boolean, "C");
    c.add("representatives", Opt::Boolean, "R");
    c.add("best", Opt::Boolean, "B");
    c.add("tree", Opt::Boolean, "T");
    c.add("assign", Opt::File, "A");
    c.add("medoid", Opt::Boolean, "M");
    c.add("complete", Opt::Boolean, "L");
    c.add("density", Opt::Integer, "D", "", 1, (float)0x7FFFFFFF);
    c.add("pvalue", Opt::Number, "v", "1.0", 0., 1.);
    c.add("distance", Opt::Number, "d", "0.05", 0., 1.);
    c.use_sketch_options();
    if (c.parse(argc, argv)) return 1;
    if (c.args.empty() || c.o("help").active) {
        cout << "\nUsage:\n\n  mash cluster [options] <seq1> [<seq2>] ...\n\n"
                "Single-linkage clusters of the pairs that `mash triangle -E` prints under the same -d and -v.\n"
                "Output fields, one line per sketch in input order: [cluster-number, cluster-size, ID]; clusters are\n"
                "numbered from 1 in order of their first member, which is the cluster's representative.\n"
                "Options: -l -C and the sketch options of `mash sketch`.\n"
                "  -d <num>  Maximum distance of an edge (0-1) [0.05]\n"
                "  -v <num>  Maximum p-value of an edge (0-1) [1.0]\n"
                "  -R        Greedy representative clusters instead of single linkage: in input order, a sketch\n"
                "            becomes a representative if no earlier representative has an edge to it, and joins the\n"
                "            first representative that has one otherwise.  No two representatives share an edge and\n"
                "            every member has an edge to its representative.\n"
                "  -B        The representatives of -R (implied), but every other sketch joins its nearest representative:\n"
                "            among all representatives it has an edge to, earlier or later in the input, the one with the\n"
                "            larger shared-hashes as an exact fraction; equal fractions go to the earlier representative.\n"
                "            Output gets a fourth field, [cluster-number, cluster-size, ID, representative-ID]: a member\n"
                "            may precede its representative.  Clusters are numbered by their representatives' order.  Not\n"
                "            with -T.  Not with -A: a new representative can be nearer to an earlier member than the one it\n"
                "            was filed under, and that pair is not among those -A compares.\n"
                "  -T        The minimum spanning forest of those pairs instead of clusters: one `mash triangle -E` line\n"
                "            per forest edge, best first by shared-hashes as an exact fraction, equal fractions in the\n"
                "            order of `mash triangle -E`.  The lines down to any fraction are the forest, and give the\n"
                "            single-linkage clusters, of that stricter threshold.  Not with -R.\n"
                "  -A <file> Extend an earlier clustering: <file> is the output of an earlier `mash cluster` (or `mash\n"
                "            cluster -R`, then give -R again) over the FIRST inputs, one line each; the IDs must match.  Only\n"
                "            pairs with one of the later inputs are compared.  All inputs are listed; if <file> was made\n"
                "            with the same -R, -d and -v, the output is that of the run without -A, and it can be given\n"
                "            to the next -A.  The mode and thresholds behind <file> are not checked.  Not with -T.\n"
                "  -M        The single-linkage clusters with each cluster's medoid: output gets a fourth field,\n"
                "            [cluster-number, cluster-size, ID, medoid-ID]; the first three fields are those of the run\n"
                "            without -M.  An edge weighs floor(shared * 2^32 / max(denominator, 1)) with shared/denominator\n"
                "            the shared-hashes of its `mash triangle -E` line, a sketch's score is the sum over its edges (a\n"
                "            pair of the cluster that is no edge counts 0), and the medoid is the member with the largest\n"
                "            score, equal scores to the earlier member: with full sketches, the member with the largest mean\n"
                "            Jaccard estimate to the rest of its cluster.  Exact integers throughout.  Not with -R, -B, -T\n"
                "            or -A (the weights between earlier inputs are not among the pairs -A compares).\n"
                "  -L        Complete-linkage clusters instead of single linkage: every two members of a cluster share an\n"
                "            edge.  Two clusters are linked if every pair between them is an edge, and the link weighs what\n"
                "            its worst pair does: the smallest shared-hashes as an exact fraction.  Starting from single\n"
                "            sketches, the best link is merged, equal fractions going to the link whose later cluster comes\n"
                "            first in the input, then to the one whose earlier cluster does, until no link is left.  The\n"
                "            result depends on the edges and their shared-hashes alone.  Output fields and numbering are\n"
                "            those of the plain run.  Not with -R, -B, -M or -T.  Not with -A: merges among the earlier\n"
                "            inputs are not a function of the pairs -A compares.\n"
                "  -D <int>  Density clusters (DBSCAN) instead of single linkage (1-2147483647).  A sketch with at least <int>\n"
                "            edges, that is <int> OTHER sketches within the threshold, is a core (the classic minPts, which\n"
                "            counts the sketch itself, is <int> + 1).  Clusters are the connected components of the cores\n"
                "            under the edges between two cores.  Any other sketch with an edge to a core is a border and joins\n"
                "            the cluster of its nearest core: the larger shared-hashes as an exact fraction, equal fractions to\n"
                "            the earlier core.  A border never joins two clusters, so a thin bridge between two groups does\n"
                "            not chain them.  The rest is noise, each a cluster of its own.  Output gets two more fields,\n"
                "            [cluster-number, cluster-size, ID, role, neighbours]: role is core, border or noise, neighbours\n"
                "            the number of the sketch's edges.  Numbering is that of the plain run, from 1 by first member;\n"
                "            with -D 1 the first three fields are the plain run's.  Not with -R, -B, -T, -A, -M or -L.\n\n";
        return 0;
    }
    const bool comment = c.o("comment").active, extend = c.o("assign").active;
    const double p_max = c.o("pvalue").num, d_max = c.o("distance").num;
    // what cannot be given together, in order of precedence: the first row that matches is the one reported
    static const struct { const char *a, *b, *why; } refusals[] = {
        {"medoid", "representatives", ""}, {"medoid", "best", ""}, {"medoid", "tree", ""},
        {"medoid", "assign", " (the weights between earlier inputs are not among the pairs -A compares)"},
        {"best", "tree", ""}, {"best", "assign", " (a new representative can be nearer to an earlier member)"},
        {"tree", "representatives", ""}, {"tree", "assign", ""},
        {"complete", "representatives", ""}, {"complete", "best", ""}, {"complete", "medoid", ""}, {"complete", "tree", ""}, {"complete", "assign", ""},
        {"density", "representatives", ""}, {"density", "best", ""}, {"density", "tree", ""},
        {"density", "assign", " (a new input changes the degrees, and so the roles, of earlier ones)"}, {"density", "medoid", ""}, {"density", "complete", ""},
    };
    for (const auto &x : refusals) {
        if (!c.o(x.a).active || !c.o(x.b).active) continue;
        cerr << "ERROR: -" << c.o(x.a).id << " and -" << c.o(x.b).id << " cannot be given together" << x.why << "." << endl;
        return 1;
    }
    if (d_max >= 1.0 && p_max >= 1.0) {
        cerr << "ERROR: With -" << c.o("distance").id << " 1 and -" << c.o("pvalue").id << " 1 every pair is an edge; give a smaller maximum." << endl;
        return 1;
    }
    Params p;
    if (sketch_parameter_setup(p, c)) return 1;
    if (c.args.size() == 1 && !c.o("list").active) p.concatenated = false;   // as `mash triangle` (CommandTriangle.cpp:74-77)
    // (-D: the option holds a float, exact to 2^24 only: the count is read from the text the parser has accepted)
    const uint64_t min_nb = c.o("density").active ? strtoull(c.o("density").arg.c_str(), nullptr, 10) : 0;
    if (c.o("density").active && (min_nb < 1 || min_nb > 0x7FFFFFFFull)) {
        cerr << "ERROR: Argument to -" << c.o("density").id << " must be an integer between 1 and 2147483647 (" << c.o("density").arg << " given)" << endl;
        return 1;
    }
    const ClusterMode mode = c.o("density").active ? kDensity : c.o("complete").active ? kComplete : c.o("tree").active ? kForest : c.o("medoid").active ? kMedoid : c.o("best").active ? kNearest
                             : c.o("representatives").active ? kGreedy : kSingle;
    Earlier old;
    if (extend && !read_earlier(c.o("assign").arg, old)) return 1;           // (before a device is opened)
    Gpu gpu;
    SketchSet set;
    init_from_files(gpu, set, input_files(c), p, 1);
    const KmerWarning w = scan_kmer_warning(set);
    const uint64_t n = set.refs.size();
    auto label = [&](uint64_t i) -> const string & { return comment ? set.refs[i].comment : set.refs[i].name; };      // (TriRun::label, for -A too)
    if (extend) {
        if (old.id.size() > n) {
            cerr << "ERROR: " << c.o("assign").arg << " has " << old.id.size() << " lines, but there are only " << n << " input sequences." << endl;
            return 1;
        }
        for (uint64_t i = 0; i < old.id.size(); i++) {
            const string &id = label(i);
            if (id == old.id[i]) continue;
            cerr << "ERROR: Line " << (i + 1) << " of " << c.o("assign").arg << " is about \"" << old.id[i] << "\", but input " << (i + 1) << " is \"" << id
                 << "\": the earlier inputs must come first, in the same order." << endl;
            return 1;
        }
    }
    if (n == 0) return 0;
    Clusters found{vector<uint32_t>(n), vector<uint32_t>(mode == kMedoid ? n : 0), {}, (uint32_t)min_nb, vector<uint32_t>(mode == kDensity ? n : 0),
                   vector<uint32_t>(mode == kDensity ? n : 0)};
    auto print_clusters = [&](FastOut &out) {
        // label = the cluster's first member: numbers in order of first appearance are numbers by ascending label
        const vector<uint32_t> &lab = found.lab, &med = found.med;
        vector<uint32_t> number(n, 0), size(n, 0);
        uint32_t next = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (lab[i] == i) number[i] = ++next;
            size[lab[i]]++;
        }
        for (uint64_t i = 0; i < n; i++) {
            out << number[lab[i]] << '\t' << size[lab[i]] << '\t' << label(i);
            if (mode == kNearest) out << '\t' << label(lab[i]);
            if (mode == kMedoid) out << '\t' << label(med[i]);
            if (mode == kDensity) out << '\t' << (found.deg[i] >= min_nb ? "core" : found.via[i] != i ? "border" : "noise") << '\t' << found.deg[i];
            out.eol();
        }
    };
    if (extend) {
        StageClock clk;                                          // (-A uploads two tables of its own, inside its first lap)
        FastOut out;
        if (cluster_extend(gpu, set, old, mode, d_max, p_max, clk, found)) return 1;
        print_clusters(out);
        clk.lap("format+write");
        return finish_run(set, w, p.reads);
    }
    TriRun run(gpu, set, comment, true, 0, d_max, p_max);
    if (cluster_table(run, mode, found)) return 1;
    if (mode == kForest) tri_emit_results(run, found.forest);
    else print_clusters(run.out);
    run.clk.lap("format+write");
    run.dt.reset();                                              // (inside the "teardown" lap, as the later lines)
    return finish_run(set, w, p.reads);
}

void print_columns(const vector<vector<string>> &cols, int indent, int spacing, const char *missing)
{
    vector<size_t> width(cols.size(), 0);
    for (size_t i = 0; i < cols.size(); i++)
        for (const string &s : cols[i]) width[i] = std::max(width[i], std::max<size_t>(s.size(), 1));
    for (size_t r = 0; r < cols[0].size(); r++) {
        size_t offset = 0, target = indent;
        for (size_t j = 0; j < cols.size(); j++) {
            for (size_t k = offset; k < target; k++) cout << ' ';
            const string text = cols[j][r].empty() ? string(missing) : cols[j][r];
            cout << text;
            offset = target + text.size();
            target += width[j] + spacing;
        }
        cout << endl;
    }
}

int cmd_info(int argc, const char **argv)
{
    Cmd c;
    c.name = "info";
    c.add("help", Opt::Boolean, "h");
    c.add("header", Opt::Boolean, "H");
    c.add("tabular", Opt::Boolean, "t");
    c.add("counts", Opt::Boolean, "c");
    c.add("dump", Opt::Boolean, "d");
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() != 1 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash info [options] <sketch>\n\nOptions: -H (header only) -t (tabular) -c (count histograms) -d (JSON dump)\n\n";
        return 0;
    }
    const bool header = c.o("header").active, tabular = c.o("tabular").active, counts = c.o("counts").active, dump = c.o("dump").active;
    auto incompatible = [](const char *a, const char *b) { cerr << "ERROR: The options " << a << " and " << b << " are incompatible." << endl; return 1; };
    if (header && tabular) return incompatible("-H", "-t");
    if (header && counts) return incompatible("-H", "-c");
    if (tabular && counts) return incompatible("-t", "-c");
    if (dump && tabular) return incompatible("-d", "-t");
    if (dump && header) return incompatible("-d", "-H");
    if (dump && counts) return incompatible("-d", "-c");
    const string &file = c.args[0];
    if (!has_suffix(file, kSuffix)) { cerr << "ERROR: The file \"" << file << "\" does not look like a sketch." << endl; return 1; }
    mshio::File f;
    const string e = mshio::read_msh(file, f, header);
    if (!e.empty()) { cerr << "ERROR: " << e << endl; return 1; }
    Params p;
    params_from_header(p, f.header);
    const uint64_t nref = header ? f.header.reference_count : f.references.size();
    if (counts) {
        if (f.references.empty()) { cerr << "ERROR: Sketch file contains no sketches" << endl; return 1; }
        if (!f.header.has_counts) { cerr << "ERROR: Sketch file does not have hash counts. Re-sketch with -M to use this feature." << endl; return 1; }
        cout << "#Sketch\tBin\tFrequency" << endl;
        for (const auto &r : f.references) {
            std::map<uint32_t, uint64_t> hist;
            for (uint32_t v : r.counts) hist[v]++;
            for (const auto &kv : hist) cout << r.name << '\t' << kv.first << '\t' << kv.second << endl;
        }
        return 0;
    }
    if (dump) {                                              // writeJson, CommandInfo.cpp:222-299 (byte for byte)
        cout << "{" << endl;
        cout << "	\"kmer\" : " << p.kmer << ',' << endl;
        cout << "	\"alphabet\" : \"" << p.alphabet << "\"," << endl;
        cout << "	\"preserveCase\" : " << (p.preserve_case ? "true" : "false") << ',' << endl;
        cout << "	\"canonical\" : " << (p.noncanonical ? "false" : "true") << ',' << endl;
        cout << "	\"sketchSize\" : " << p.sketch_size << ',' << endl;
        cout << "	\"hashType\" : \"MurmurHash3_x64_128\"," << endl;
        cout << "	\"hashBits\" : " << (p.use64 ? 64 : 32) << ',' << endl;
        cout << "	\"hashSeed\" : " << p.seed << ',' << endl;
        cout << " 	\"sketches\" :" << endl;
        cout << "	[" << endl;
        for (size_t i = 0; i < f.references.size(); i++) {
            const auto &r = f.references[i];
            cout << "		{" << endl;
            cout << "			\"name\" : \"" << r.name << "\"," << endl;
            cout << "			\"length\" : " << r.length << ',' << endl;
            cout << "			\"comment\" : \"" << r.comment << "\"," << endl;
            cout << "			\"hashes\" :" << endl;
            cout << "			[" << endl;
            for (size_t j = 0; j < r.hashes.size(); j++) {
                cout << "				" << r.hashes[j];
                if (j + 1 < r.hashes.size()) cout << ',';
                cout << endl;
            }
            cout << "			]" << endl;
            if (r.counts_sorted) {
                cout << "			\"counts\" :" << endl;
                cout << "			[" << endl;
                for (size_t j = 0; j < r.counts.size(); j++) {
                    cout << "				" << r.counts[j];
                    if (j + 1 < r.hashes.size()) cout << ',';
                    cout << endl;
                }
                cout << "			]" << endl;
            }
            cout << (i + 1 < f.references.size() ? "		}," : "		}") << endl;
        }
        cout << "	]" << endl;
        cout << "}" << endl;
        return 0;
    }
    if (tabular) {
        cout << "#Hashes\tLength\tID\tComment" << endl;
    } else {
        cout << "Header:" << endl;
        cout << "  Hash function (seed):          MurmurHash3_x64_128 (" << p.seed << ")" << endl;
        cout << "  K-mer size:                    " << p.kmer << " (" << (p.use64 ? "64" : "32") << "-bit hashes)" << endl;
        cout << "  Alphabet:                      " << p.alphabet << (p.noncanonical ? "" : " (canonical)") << (p.preserve_case ? " (case-sensitive)" : "") << endl;
        cout << "  Target min-hashes per sketch:  " << p.sketch_size << endl;
        cout << "  Sketches:                      " << nref << endl;
    }
    if (!header) {
        vector<vector<string>> cols(4);
        if (!tabular) {
            cout << endl << "Sketches:" << endl;
            cols[0].push_back("[Hashes]"); cols[1].push_back("[Length]"); cols[2].push_back("[ID]"); cols[3].push_back("[Comment]");
        }
        for (const auto &r : f.references) {
            if (tabular) cout << r.hashes.size() << '\t' << r.length << '\t' << r.name << '\t' << r.comment << endl;
            else {
                cols[0].push_back(std::to_string(r.hashes.size()));
                cols[1].push_back(std::to_string(r.length));
                cols[2].push_back(r.name);
                cols[3].push_back(r.comment);
            }
        }
        if (!tabular) print_columns(cols, 2, 2, "-");
    }
    return 0;
}

int cmd_paste(int argc, const char **argv)
{
    Cmd c;
    c.name = "paste";
    c.add("help", Opt::Boolean, "h");
    c.add("list", Opt::Boolean, "l");
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() < 2 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash paste [options] <out_prefix> <sketch> [<sketch>] ...\n\nOptions: -l (inputs are lists of file names)\n\n";
        return 0;
    }
    vector<string> files;
    for (size_t i = 1; i < c.args.size(); i++) { if (c.o("list").active) split_file(c.args[i], files); else files.push_back(c.args[i]); }
    for (const string &f : files)
        if (!has_suffix(f, kSuffix)) { cerr << "ERROR: The file \"" << f << "\" does not look like a sketch." << endl; return 1; }
    SketchSet set;
    for (size_t i = 0; i < files.size(); i++) load_msh_into(set, files[i], i == 0);
    string out = c.args[0];
    if (!has_suffix(out, kSuffix)) out += kSuffix;
    if (access(out.c_str(), F_OK) != -1) { cerr << "ERROR: \"" << out << "\" exists; remove to write." << endl; exit(1); }
    cerr << "Writing " << out << "..." << endl;
    const string e = write_set(set, out);
    if (!e.empty()) { cerr << "ERROR: " << e << endl; return 1; }
    return 0;
}

// The pool of `mash screen` and `mash taxscreen`: args[1..] are its files ("-" = stdin, first only); records are read round
// robin over the inputs (CommandScreen.cpp:197-270), those shorter than k dropped, and handed to `add` in batches joined
// with MG_RECORD_SEP.  Returns the number of records seen.
uint64_t stream_pools(const vector<string> &args, int kmer, const std::function<void(const uint8_t *, size_t)> &add)
{
    const int nq = (int)args.size() - 1;
    vector<fastx::Reader *> readers;
    for (int f = 1; f <= nq; f++) {
        if (args[f] == "-" && f > 1) { cerr << "ERROR: '-' for stdin must be first query" << endl; exit(1); }
        fastx::Reader *r = new fastx::Reader;
        if (!r->open(args[f])) { cerr << "ERROR: could not open " << args[f] << endl; exit(1); }
        readers.push_back(r);
    }
    vector<uint8_t> batch;
    batch.reserve(256u << 20);
    size_t screen_batch_bytes = 255u << 20;
    if (const char *e = getenv("MASH_AMD_SCREEN_BATCH")) screen_batch_bytes = std::max<size_t>(64, strtoull(e, nullptr, 10));   // test knob
    auto flush = [&]() {
        if (batch.empty()) return;
        add(batch.data(), batch.size());
        batch.clear();
    };
    fastx::Record rec;
    size_t it = 0;
    long l = -1;
    uint64_t count = 0;
    while (!readers.empty()) {
        l = readers[it]->next(rec);
        if (l < -1) break;
        if (l == -1) {
            delete readers[it];
            readers.erase(readers.begin() + it);
            if (it == readers.size()) it = 0;
            continue;
        }
        count++;
        if (l >= kmer) {
            batch.insert(batch.end(), rec.seq.begin(), rec.seq.end());
            batch.push_back((uint8_t)MG_RECORD_SEP);
            if (batch.size() > screen_batch_bytes) flush();
        }
        it++;
        if (it == readers.size()) it = 0;
    }
    for (auto *r : readers) delete r;
    if (l != -1) { cerr << "\nERROR: reading inputs" << endl; exit(1); }
    flush();
    return count;
}

// mash screen (CommandScreen.cpp:54-461).  One device: the rows come finished from libmashgpu (mg_screen_results_host: shared,
// winners, medians, identity, p-value and both filters on the device).  Several devices, or MASH_AMD_HOST_SCREEN_FINISH=1
// (test knob, the counterpart of MASH_AMD_HOST_FINISH): the sharded screen's sparse hits and the tail on the host.
int cmd_screen(int argc, const char **argv)
{
    Cmd c;
    c.name = "screen";
    c.add("help", Opt::Boolean, "h");
    c.add("threads", Opt::Integer, "p", "1");
    c.add("winning!", Opt::Boolean, "w");
    c.add("identity", Opt::Number, "i", "0", -1., 1.);
    c.add("pvalue", Opt::Number, "v", "1.0", 0., 1.);
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() < 2 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash screen [options] <queries>.msh <mixture> [<mixture>] ...\n\n"
                "Output fields: [identity, shared-hashes, median-multiplicity, p-value, query-ID, query-comment].\n"
                "Options: -w (winner-takes-all) -i <min identity> -v <max p-value>\n\n";
        return 0;
    }
    if (!has_suffix(c.args[0], kSuffix)) { cerr << "ERROR: " << c.args[0] << " does not look like a sketch (.msh)" << endl; exit(1); }
    const double p_max = c.o("pvalue").num, identity_min = c.o("identity").num;
    SketchSet set;
    load_msh_into(set, c.args[0], true);
    const bool trans = set.p.alphabet == normalise_alphabet(kAlphabetProtein, false);   // CommandScreen.cpp:120
    StageClock clk;
    Gpu gpu;
    cerr << "Loading " << c.args[0] << "..." << endl;
    const uint64_t n = set.refs.size(), s = set.p.sketch_size;
    // the query table on every GPU; the mixture is sharded by batch over them (mg_dscreen)
    mg_dtable *t = upload_all(gpu, set, s);
    mg_params mp;
    mg_params_init(&mp, set.p.kmer, s, set.p.seed, set.p.alphabet.c_str(), set.p.noncanonical, set.p.preserve_case);
    clk.lap("device");
    const int nq = (int)c.args.size() - 1;
    const double kspace = set.kmer_space();
    const bool winner = c.o("winning!").active;
    auto announce = [&](uint64_t distinct, uint64_t count, uint64_t set_size) {
        cerr << "   " << distinct << " distinct hashes." << endl;
        cerr << (trans ? "Translating from " : "Streaming from ");
        if (nq == 1) cerr << c.args[1]; else cerr << nq << " inputs";
        cerr << "..." << endl;
        if (count == 0) { cerr << "\nERROR: Did not find sequence records in inputs" << endl; exit(1); }
        cerr << "   Estimated distinct" << (trans ? " (translated)" : "") << " k-mers in mixture: " << set_size << endl;
        if (set_size == 0) cerr << "WARNING: no valid k-mers in input." << endl;
    };
    if (mg_comm_size(gpu.comm) == 1 && !getenv("MASH_AMD_HOST_SCREEN_FINISH")) {
        auto die = [&]() { cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); };
        mg_screen *sc = nullptr;
        if ((trans ? mg_screen_create_translated(gpu.ctx, &mp, mg_dtable_local(t, 0), &sc) : mg_screen_create(gpu.ctx, &mp, mg_dtable_local(t, 0), &sc)) != MG_OK) die();
        const uint64_t count = stream_pools(c.args, set.p.kmer, [&](const uint8_t *b, size_t nb) { if (mg_screen_add_host(sc, b, nb) != MG_OK) die(); });
        clk.lap("screen");
        uint64_t nrows = 0, set_size = 0, distinct = 0;
        if (mg_screen_results_host(sc, kspace, winner ? 1 : 0, identity_min, p_max, nullptr, 0, &nrows, &set_size, nullptr, nullptr, &distinct) != MG_OK) die();
        vector<mg_screen_result> rows(nrows);
        if (nrows && mg_screen_results_host(sc, kspace, winner ? 1 : 0, identity_min, p_max, rows.data(), nrows, &nrows, nullptr, nullptr, nullptr, nullptr) != MG_OK) die();
        mg_screen_free(sc);
        mg_dtable_free(t);
        clk.lap("results");
        announce(distinct, count, set_size);
        cerr << "Summing shared..." << endl;
        if (winner) cerr << "Reallocating to winners..." << endl;
        cerr << "Computing coverage medians..." << endl;
        cerr << "Writing output..." << endl;
        for (const mg_screen_result &r : rows)
            cout << r.identity << '\t' << r.shared << '/' << r.denom << '\t' << r.median << '\t' << r.p_value << '\t' << set.refs[r.row].name << '\t'
                 << set.refs[r.row].comment << endl;
        return 0;
    }
    mg_dscreen *sc = nullptr;
    if (mg_dscreen_create(gpu.comm, &mp, t, trans ? 1 : 0, &sc) != MG_OK) {
        cerr << "ERROR: " << mg_comm_last_error(gpu.comm) << endl;
        return 1;
    }
    const uint64_t count = stream_pools(c.args, set.p.kmer, [&](const uint8_t *b, size_t nb) {
        if (mg_dscreen_add_host(sc, b, nb) != MG_OK) { cerr << "ERROR: " << mg_comm_last_error(gpu.comm) << endl; exit(1); }
    });
    // what the mixture touched: one hit per (sketch, hash) that was observed -- not the n x s matrix of
    // counters, of which a mixture leaves all but a fraction of a per cent at zero
    vector<uint64_t> mix(s);
    uint32_t mix_n = 0;
    uint64_t distinct = 0, nhits = 0;
    if (mg_dscreen_finish_sparse_host(sc, nullptr, 0, &nhits, mix.data(), &mix_n, &distinct) != MG_OK) { cerr << "ERROR: " << mg_comm_last_error(gpu.comm) << endl; return 1; }
    vector<mg_screen_hit> hits(nhits);
    if (nhits && mg_dscreen_finish_sparse_host(sc, hits.data(), nhits, &nhits, nullptr, nullptr, nullptr) != MG_OK) { cerr << "ERROR: " << mg_comm_last_error(gpu.comm) << endl; return 1; }
    mg_dscreen_free(sc);
    mg_dtable_free(t);
    clk.lap("screen");
    // estimateSetSize of the mixture's bottom-s (MinHashHeap.h:45, CommandScreen.cpp:322)
    double est = 0;
    if (mix_n) est = std::pow(2.0, set.p.use64 ? 64.0 : 32.0) * (double)mix_n / (double)mix[mix_n - 1];
    const uint64_t set_size = (uint64_t)est;
    announce(distinct, count, set_size);
    cerr << "Summing shared..." << endl;
    vector<uint64_t> shared(n, 0);
    vector<vector<uint64_t>> depths(n);
    for (const mg_screen_hit &h : hits) { shared[h.row]++; depths[h.row].push_back(h.count); }       // (ordered by sketch, then hash)
    if (winner) {
        cerr << "Reallocating to winners..." << endl;
        vector<double> scores(n);
        for (uint64_t i = 0; i < n; i++) scores[i] = mg_identity(shared[i], set.refs[i].hashes.size(), set.p.kmer);
        // each observed hash goes to the best-scoring sketch containing it (ties: larger length, then first seen)
        std::map<uint64_t, vector<uint32_t>> owners;
        std::map<uint64_t, uint32_t> obs;
        for (const mg_screen_hit &h : hits) { owners[h.hash].push_back(h.row); obs[h.hash] = h.count; }
        std::fill(shared.begin(), shared.end(), 0);
        for (auto &d : depths) d.clear();
        for (const auto &kv : owners) {
            double max_score = 0;
            uint64_t max_len = 0, max_idx = kv.second[0];
            for (uint32_t k : kv.second) {
                if (scores[k] > max_score) { max_score = scores[k]; max_idx = k; max_len = set.refs[k].length; }
                else if (scores[k] == max_score && set.refs[k].length > max_len) { max_idx = k; max_len = set.refs[k].length; }
            }
            shared[max_idx]++;
            depths[max_idx].push_back(obs[kv.first]);
        }
    }
    cerr << "Computing coverage medians..." << endl;
    for (auto &d : depths) std::sort(d.begin(), d.end());
    cerr << "Writing output..." << endl;
    for (uint64_t i = 0; i < n; i++) {
        if (shared[i] != 0 || identity_min < 0.0) {
            const uint64_t denom = set.refs[i].hashes.size();
            const double identity = mg_identity(shared[i], denom, set.p.kmer);
            if (identity < identity_min) continue;
            const double pv = mg_p_value_within(shared[i], set_size, kspace, denom);
            if (pv > p_max) continue;
            cout << identity << '\t' << shared[i] << '/' << denom << '\t' << (shared[i] > 0 ? depths[i].at(shared[i] / 2) : 0)
                 << '\t' << pv << '\t' << set.refs[i].name << '\t' << set.refs[i].comment << endl;
        }
    }
    clk.lap("host tail");
    return 0;
}

// mash taxscreen (CommandTaxScreen.cpp:57-474): a screen whose result is a Kraken-style report over a taxonomy.  One device:
// the per-hash LCA, the per-taxon histograms and the clade sums are libmashgpu's (mg_screen_set_taxa / mg_screen_tax_finish_host).
int cmd_taxscreen(int argc, const char **argv)
{
    Cmd c;
    c.name = "taxscreen";
    c.add("help", Opt::Boolean, "h");
    c.add("threads", Opt::Integer, "p", "1");
    c.add("identity", Opt::Number, "i", "0", -1., 1.);      // read and never used by the reference (:75-76): accepted, no effect
    c.add("pvalue", Opt::Number, "v", "1.0", 0., 1.);
    c.add("mapping-file", Opt::String, "m", "");
    c.add("taxonomy-dir", Opt::String, "t", ".");
    if (c.parse(argc, argv)) return 1;
    if (c.args.size() < 2 || c.o("help").active) {
        cout << "\nUsage:\n\n  mash taxscreen [options] <queries>.msh <pool> [<pool>] ...\n\n"
                "Kraken-style taxonomic report of how well the query sketches are contained in a pool of sequences.\n"
                "Output fields: [total percent of hashes, contained hashes in the clade, contained hashes in the taxon,\n"
                "hashes in the clade, hashes in the taxon, rank, taxonomy ID, padded name].\n"
                "Options: -m <mapping file: taxid, one separator, reference name> -t <directory with nodes.dmp and names.dmp>\n"
                "         -p <threads> -i <min identity> -v <max p-value> (the last three are accepted and change nothing)\n\n";
        return 0;
    }
    if (!has_suffix(c.args[0], kSuffix)) { cerr << "ERROR: " << c.args[0] << " does not look like a sketch (.msh)" << endl; exit(1); }
    SketchSet set;
    load_msh_into(set, c.args[0], true);
    const bool trans = set.p.alphabet == normalise_alphabet(kAlphabetProtein, false);
    const string dir = c.o("taxonomy-dir").arg, names_file = dir + "/names.dmp", nodes_file = dir + "/nodes.dmp";
    if (!std::ifstream(names_file).good() || !std::ifstream(nodes_file).good()) {
        cerr << "Could not find a file names.dmp or nodes.dmp in directory " << dir << "\n"
             << " The NCBI taxonomy dump (taxdump.tar.gz, pub/taxonomy on the NCBI FTP server) holds both.\n" << endl;
        exit(1);
    }
    cerr << "Loading taxonomy files ..." << endl;
    taxdb::Taxonomy tax;
    string err;
    if (!tax.load(nodes_file, names_file, &err)) { cerr << "ERROR: " << err << endl; exit(1); }
    cerr << "   " << tax.nodes.size() << " distinct taxa\n";
    cerr << "Reading mapping file ..." << endl;
    const uint64_t n = set.refs.size(), s = set.p.sketch_size;
    vector<string> names(n), comments(n);
    for (uint64_t i = 0; i < n; i++) { names[i] = set.refs[i].name; comments[i] = set.refs[i].comment; }
    vector<uint64_t> row_taxid;
    if (!taxdb::reference_taxids(names, comments, c.o("mapping-file").arg, &row_taxid)) { cerr << "ERROR: unable to open mapping file" << endl; exit(1); }
    for (uint64_t i = 0; i < n; i++)
        if (row_taxid[i] == 0) cerr << "Could not find taxID for reference " << names[i] << " in comment field or mapping file!" << endl;
    const taxdb::Binding bind(tax, row_taxid);
    Gpu gpu;
    cerr << "Loading " << c.args[0] << "..." << endl;
    mg_dtable *t = upload_all(gpu, set, s);
    mg_params mp;
    mg_params_init(&mp, set.p.kmer, s, set.p.seed, set.p.alphabet.c_str(), set.p.noncanonical, set.p.preserve_case);
    auto die = [&]() { cerr << "ERROR: " << mg_last_error(gpu.ctx) << endl; exit(1); };
    mg_screen *sc = nullptr;
    mg_taxonomy *mt = nullptr;
    if ((trans ? mg_screen_create_translated(gpu.ctx, &mp, mg_dtable_local(t, 0), &sc) : mg_screen_create(gpu.ctx, &mp, mg_dtable_local(t, 0), &sc)) != MG_OK) die();
    cerr << "Assigning LCA taxIDs to hashes ..." << endl;    // (once per database, before the pool is read: it does not depend on it)
    if (mg_taxonomy_create(gpu.ctx, bind.parent.data(), bind.parent.size(), &mt) != MG_OK) die();
    if (mg_screen_set_taxa(sc, mt, bind.row_node.data(), n) != MG_OK) die();
    const int nq = (int)c.args.size() - 1;
    cerr << (trans ? "Translating from " : "Streaming from ");
    if (nq == 1) cerr << c.args[1]; else cerr << nq << " inputs";
    cerr << "..." << endl;
    const uint64_t count = stream_pools(c.args, set.p.kmer, [&](const uint8_t *b, size_t nb) { if (mg_screen_add_host(sc, b, nb) != MG_OK) die(); });
    vector<uint64_t> mix(s);
    uint32_t mix_n = 0;
    uint64_t distinct = 0, ntaxa = 0, total = 0, total_hash = 0;
    if (mg_screen_tax_finish_host(sc, nullptr, 0, &ntaxa, nullptr, nullptr, nullptr, nullptr, nullptr) != MG_OK) die();
    vector<mg_taxon_count> taxa(ntaxa);
    if (mg_screen_tax_finish_host(sc, taxa.data(), ntaxa, &ntaxa, &total, &total_hash, mix.data(), &mix_n, &distinct) != MG_OK) die();
    mg_screen_free(sc);
    mg_taxonomy_free(mt);
    mg_dtable_free(t);
    cerr << "   " << distinct << " distinct hashes." << endl;
    if (count == 0) { cerr << "\nERROR: Did not find sequence records in inputs" << endl; exit(1); }
    double est = 0;
    if (mix_n) est = std::pow(2.0, set.p.use64 ? 64.0 : 32.0) * (double)mix_n / (double)mix[mix_n - 1];
    cerr << "   Estimated distinct" << (trans ? " (translated)" : "") << " k-mers in pool: " << (uint64_t)est << endl;
    if ((uint64_t)est == 0) cerr << "WARNING: no valid k-mers in input." << endl;
    cerr << "Writing output..." << endl;
    taxdb::write_report(stdout, tax, taxdb::counts_by_taxid(tax, bind, taxa.data(), ntaxa), total);
    return 0;
}

// mash bounds (CommandBounds.cpp:33-136): a table of error bounds, host arithmetic only
int cmd_bounds(int argc, const char **argv)
{
    Cmd c;
    c.name = "bounds";
    c.add("help", Opt::Boolean, "h");
    c.add("kmer", Opt::Integer, "k", "21", 1, 32);
    c.add("prob", Opt::Number, "p", "0.99", 0, 1);
    if (c.parse(argc, argv)) return 1;
    if (c.o("help").active) {
        cout << "\nUsage:\n\n  mash bounds [options]\n\nPrint a table of Mash error bounds for various sketch sizes and Mash distances.\n"
                "Options: -k <k-mer size> -p <probability that an estimate is within the bounds>\n\n";
        return 0;
    }
    const int sketch_sizes[] = {100, 500, 1000, 5000, 10000, 50000, 100000, 500000, 1000000};
    const double dists[] = {0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4};
    const int k = (int)c.o("kmer").num;
    const double q2 = (1.0 - c.o("prob").num) / 2.0;
    cout << endl << "Parameters (run with -h for details):" << endl;
    cout << "   k:   " << k << endl;
    cout << "   p:   " << c.o("prob").num << endl << endl;
    for (int cont = 0; cont < 2; cont++) {
        cout << (cont ? "\tScreen distance" : "\tMash distance") << endl;
        cout << "Sketch";
        for (double d : dists) cout << '\t' << d;
        cout << endl;
        for (int s : sketch_sizes) {
            cout << s;
            for (double d : dists) {
                const double m2j = cont ? pow(1.0 - d, k) : 1.0 / (2.0 * exp(k * d) - 1.0);
                // the least x < s with P(X <= x) > q2, else s.  P(X <= x) = 1 - P(X > x) does not fall as x grows, so the
                // reference's scan from 0 and a bisection find the same x.
                int lo = 0, hi = s;
                while (lo < hi) {
                    const int x = lo + (hi - lo) / 2;
                    if (1.0 - mg::binomial_q((uint64_t)x, m2j, (uint64_t)s) > q2) hi = x; else lo = x + 1;
                }
                const double je = double(lo) / s;
                const double j2m = cont ? 1.0 - pow(je, 1. / k) : -1.0 / k * log(2.0 * je / (1.0 + je));
                cout << '\t' << j2m - d;
            }
            cout << endl;
        }
        cout << endl;
    }
    return 0;
}

// test/interchange helper: rebuild a .msh from the JSON `mash info -d` prints (no GPU)
int cmd_json2msh(int argc, const char **argv)
{
    if (argc != 2) { cerr << "usage: mash json2msh <info-dump.json> <out.msh>" << endl; return 1; }
    std::ifstream in(argv[0]);
    if (in.fail()) { cerr << "ERROR: Could not open " << argv[0] << endl; return 1; }
    string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    auto find_value = [&](size_t from, const string &key, size_t *at) -> string {
        const string pat = "\"" + key + "\" :";
        size_t p = text.find(pat, from);
        if (p == string::npos) { *at = string::npos; return ""; }
        p += pat.size();
        while (p < text.size() && (text[p] == ' ' || text[p] == '\n' || text[p] == '\t')) p++;
        size_t e;
        string v;
        if (text[p] == '"') { e = text.find("\",\n", p + 1); if (e == string::npos) e = text.find("\"\n", p + 1); v = text.substr(p + 1, e - p - 1); }
        else { e = text.find_first_of(",\n", p); v = text.substr(p, e - p); }
        *at = e;
        return v;
    };
    size_t at;
    mshio::File f;
    f.header.kmer_size = (uint32_t)std::stoul(find_value(0, "kmer", &at));
    f.header.alphabet = find_value(0, "alphabet", &at);
    f.header.has_alphabet = true;
    f.header.preserve_case = find_value(0, "preserveCase", &at) == "true";
    f.header.noncanonical = find_value(0, "canonical", &at) != "true";
    f.header.sketch_size = (uint32_t)std::stoul(find_value(0, "sketchSize", &at));
    f.header.seed = (uint32_t)std::stoul(find_value(0, "hashSeed", &at));
    f.header.concatenated = true;
    size_t pos = text.find("\"sketches\"");
    while (true) {
        size_t a1;
        const string name = find_value(pos, "name", &a1);
        if (a1 == string::npos) break;
        mshio::Reference r;
        r.name = name;
        r.length = std::stoull(find_value(a1, "length", &a1));
        r.comment = find_value(a1, "comment", &a1);
        size_t hb = text.find('[', text.find("\"hashes\"", a1)), he = text.find(']', hb);
        const char *q = text.c_str() + hb + 1, *qe = text.c_str() + he;
        while (q < qe) {
            while (q < qe && (*q < '0' || *q > '9')) q++;
            if (q >= qe) break;
            char *end;
            r.hashes.push_back(strtoull(q, &end, 10));
            q = end;
        }
        f.references.push_back(std::move(r));
        pos = he;
    }
    const string e = mshio::write_msh(argv[1], f);
    if (!e.empty()) { cerr << "ERROR: " << e << endl; return 1; }
    return 0;
}

}  // namespace

int main(int argc, const char **argv)
{
    const string usage =
        "\nMash (MI355X hot path), commands:\n\n  sketch    Create sketches (reduced representations for fast operations).\n"
        "  dist      Estimate the distance of query sequences to references, or the spectrum of those distances (-H).\n"
        "  within    Estimate the containment of query sequences within references.\n"
        "  triangle  Estimate a lower-triangular distance matrix, or the spectrum of its distances (-H).\n"
        "  cluster   Group sequences into single-linkage or greedy representative (-R) clusters by distance, file members under their nearest representative (-B), name each single-linkage cluster's medoid (-M), extend an earlier clustering by new sequences (-A), print the minimum spanning forest (-T), form complete-linkage clusters, every two members within the distance (-L), or form density clusters of cores, borders and noise (-D).\n  info      Display information about sketch files.\n"
        "  paste     Create a single sketch file from multiple sketch files.\n"
        "  screen    Determine whether query sequences are within a larger mixture of sequences.\n"
        "  taxscreen Create Kraken-style taxonomic report based on mash screen.\n"
        "  bounds    Print a table of Mash error bounds.\n\n";
    if (argc < 2) { cout << usage; return 0; }
    const string cmd = argv[1];
    const bool timing = getenv("MASH_AMD_TIMING") != nullptr;
    auto stamp = [&](const char *what) {             // CLOCK_MONOTONIC, comparable with the caller's clock (tools/cli_e2e.py)
        if (timing) cerr << "timing: " << what << ' ' << std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() << endl;
    };
    cerr.precision(12);
    stamp("main_begin");
    cerr.precision(6);
    int rc;
    if (cmd == "sketch") rc = cmd_sketch(argc - 2, argv + 2);
    else if (cmd == "dist") rc = cmd_dist(argc - 2, argv + 2);
    else if (cmd == "within") rc = cmd_within(argc - 2, argv + 2);
    else if (cmd == "triangle") rc = cmd_triangle(argc - 2, argv + 2);
    else if (cmd == "cluster") rc = cmd_cluster(argc - 2, argv + 2);
    else if (cmd == "info") rc = cmd_info(argc - 2, argv + 2);
    else if (cmd == "paste") rc = cmd_paste(argc - 2, argv + 2);
    else if (cmd == "screen") rc = cmd_screen(argc - 2, argv + 2);
    else if (cmd == "taxscreen") rc = cmd_taxscreen(argc - 2, argv + 2);
    else if (cmd == "bounds") rc = cmd_bounds(argc - 2, argv + 2);
    else if (cmd == "json2msh") rc = cmd_json2msh(argc - 2, argv + 2);
    else if (cmd == "--version") { cout << "2.3-mi355x" << endl; rc = 0; }
    else {
        cerr << "ERROR: Unknown command: " << cmd << endl;
        cout << usage;
        rc = 1;
    }
    cerr.precision(12);
    stamp("main_end");
    // Everything this process owns is released by the kernel; unloading the HIP runtime and its code
    // objects politely takes tens of milliseconds that a caller of a 0.4 s command waits for.
    if (!getenv("MASH_AMD_SLOW_EXIT")) {
        cout.flush();
        cerr.flush();
        fflush(nullptr);
        _exit(rc);
    }
    return rc;
}
