"""Host layer: .msh codec (no libcapnp), kseq-compatible reader, `mash` CLI.
CPU tests cover the codec and the GPU-free commands (info, paste); `-m gpu` tests run the
reference's own `make test` recipe (Makefile.in:94-111) through the GPU CLI."""
import ctypes as C
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from workloads import synth
from tests import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASH = os.path.join(ROOT, "mash_amd", "bin", "mash")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(MASH) or not os.path.exists(os.path.join(ROOT, "tests", "libmshio.so")):
        g.build()
    return True


def run(*args, check=True, cwd=None, env=None):
    r = subprocess.run([MASH, *args], capture_output=True, text=True, cwd=cwd,
                       env=dict(os.environ, **env) if env else None)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def test_info_dump_reproduces_golden_json(built, tmp_path):
    """json -> .msh (our writer) -> `mash info -d` (our reader) is byte-identical to the
    reference's goldens test/ref/genomes.json and test/ref/reads.json."""
    for name in ("genomes", "reads"):
        msh = str(tmp_path / f"{name}.msh")
        run("json2msh", os.path.join(GOLD, f"{name}.json"), msh)
        out = run("info", "-d", msh).stdout
        assert out == open(os.path.join(GOLD, f"{name}.json")).read()


def test_info_header_tabular_and_paste(built, tmp_path):
    g, r = str(tmp_path / "genomes.msh"), str(tmp_path / "reads.msh")
    run("json2msh", os.path.join(GOLD, "genomes.json"), g)
    run("json2msh", os.path.join(GOLD, "reads.json"), r)
    hdr = run("info", "-H", g).stdout
    assert "K-mer size:                    21 (64-bit hashes)" in hdr
    assert "Alphabet:                      ACGT (canonical)" in hdr
    assert "Sketches:                      3" in hdr
    tab = run("info", "-t", g).stdout.splitlines()
    assert tab[0] == "#Hashes\tLength\tID\tComment"
    assert tab[1].startswith("1000\t4639675\tgenome1.fna\tgi|49175990|")
    run("paste", str(tmp_path / "all"), g, r)
    tab = run("info", "-t", str(tmp_path / "all.msh")).stdout.splitlines()
    assert len(tab) == 5 and tab[4].startswith("1000\t502359\treads\t[2000 seqs] SRR7885321.1 1 length=302 [...]")
    again = run("paste", str(tmp_path / "all"), g, r, check=False)       # refuses to overwrite (CommandPaste.cpp:79-83)
    assert again.returncode == 1 and "exists; remove to write." in again.stderr
    bad = run("info", str(tmp_path / "nosuffix"), check=False)
    assert bad.returncode == 1 and "does not look like a sketch" in bad.stderr
    inc = run("info", "-H", "-t", g, check=False)
    assert inc.returncode == 1 and "incompatible" in inc.stderr


def test_msh_wire_layout_and_foreign_encodings(built, tmp_path):
    """Wire-level checks of the hand-written codec: slot layout, seed
    default XOR, and reading what libcapnp may emit (multi-segment, far / double-far pointers)."""
    lib = C.CDLL(os.path.join(ROOT, "tests", "libmshio.so"))
    g = str(tmp_path / "genomes.msh")
    run("json2msh", os.path.join(GOLD, "genomes.json"), g)
    assert lib.mshio_roundtrip_check(g.encode()) == 0
    raw = open(g, "rb").read()
    words = np.frombuffer(raw, dtype="<u8").copy()
    assert words[0] == (len(words) - 1) << 32                  # 1 segment, its size in words
    seg = words[1:]
    rootp = int(seg[0])
    assert rootp & 3 == 0 and (rootp >> 32) & 0xFFFF == 3 and rootp >> 48 == 4      # MinHash: 3 data, 4 pointers
    assert int(seg[1]) & 0xFFFFFFFF == 21 and int(seg[2]) & 0xFFFFFFFF == 1000       # kmerSize, minHashesPerWindow
    assert int(seg[3]) >> 32 == 0                               # hashSeed 42 is stored XOR 42
    assert int(seg[4]) != 0 and int(seg[7]) == 0                # seed 42 -> referenceListOld (p0), referenceList null

    def summary(buf):
        kmer, ssz, seed = C.c_uint32(), C.c_uint32(), C.c_uint32()
        nref, h0, h1 = C.c_uint64(), C.c_uint64(), C.c_uint64()
        name = C.create_string_buffer(256)
        rc = lib.mshio_parse_summary(buf, C.c_uint64(len(buf)), C.byref(kmer), C.byref(ssz), C.byref(seed),
                                     C.byref(nref), C.byref(h0), C.byref(h1), name, C.c_uint64(256))
        return rc, kmer.value, ssz.value, seed.value, nref.value, h0.value, h1.value, name.value.decode()

    want = summary(raw)
    assert want[:5] == (0, 21, 1000, 42, 3) and want[7] == "genome1.fna"
    gh, _, _ = helpers.load_golden_genomes()
    assert want[5] == int(gh[2][0]) and want[6] == int(gh[2][-1])
    # two segments: root is a FAR pointer to a landing pad at word 0 of segment 1
    far = struct.pack("<Q", 2 | (0 << 3) | (1 << 32))
    seg1 = seg.tobytes()                                        # word 0 (the old root pointer) is the landing pad
    hdr = struct.pack("<IIII", 1, 1, len(seg), 0)
    assert summary(hdr + far + seg1) == want
    # three segments: DOUBLE-far: pad in segment 2 = {far -> seg 1 word 1, tag struct(3,4)}
    dfar = struct.pack("<Q", 2 | (1 << 2) | (0 << 3) | (2 << 32))
    pad = struct.pack("<QQ", 2 | (1 << 3) | (1 << 32), 0 | (3 << 32) | (4 << 48))
    hdr3 = struct.pack("<IIII", 2, 1, len(seg), 2)
    assert summary(hdr3 + dfar + seg1 + pad) == want
    # non-default seed moves the list to referenceList (p3) and stores seed ^ 42
    js = open(os.path.join(GOLD, "reads.json")).read().replace('"hashSeed" : 42', '"hashSeed" : 7')
    p = tmp_path / "seed7.json"
    p.write_text(js)
    m7 = str(tmp_path / "seed7.msh")
    run("json2msh", str(p), m7)
    w7 = np.frombuffer(open(m7, "rb").read(), dtype="<u8")[1:]
    assert int(w7[3]) >> 32 == (7 ^ 42) and int(w7[4]) == 0 and int(w7[7]) != 0
    assert '"hashSeed" : 7' in run("info", "-d", m7).stdout
    # truncated / corrupt files are errors, not crashes
    assert summary(raw[: len(raw) // 2 // 8 * 8])[0] == -1
    assert summary(b"\x00" * 16)[0] in (0, -1)


def test_multi_segment_writer_roundtrips_through_golden_dumps(built, tmp_path):
    """Files beyond one segment: structs stay in segment 0, lists move behind far pointers.
    Forced here with a tiny segment limit; `mash info -d` of the rewritten files still equals the
    reference's golden dumps, and the single-segment default is unchanged."""
    lib = C.CDLL(os.path.join(ROOT, "tests", "libmshio.so"))
    lib.mshio_rewrite.restype = C.c_long
    lib.mshio_rewrite.argtypes = [C.c_char_p, C.c_char_p, C.c_ulonglong]
    for name in ("genomes", "reads"):
        one = str(tmp_path / f"{name}.msh")
        run("json2msh", os.path.join(GOLD, f"{name}.json"), one)
        gold = open(os.path.join(GOLD, f"{name}.json")).read()
        for limit, min_segs in ((0, 1), (1100 if name == "genomes" else 1010, 3 if name == "genomes" else 2), (300, None)):
            out = str(tmp_path / f"{name}_{limit}.msh")
            nseg = lib.mshio_rewrite(one.encode(), out.encode(), limit)
            if min_segs is None:                                 # a 1000-hash list does not fit 300 words
                assert nseg == -2
                continue
            assert nseg >= min_segs and (limit != 0 or nseg == 1)
            assert run("info", "-d", out).stdout == gold
            assert lib.mshio_roundtrip_check(out.encode()) == 0
            if limit == 0:
                assert open(out, "rb").read() == open(one, "rb").read()
    # paste of multi-segment inputs
    a, b = str(tmp_path / "genomes_1100.msh"), str(tmp_path / "genomes_0.msh")
    run("paste", str(tmp_path / "both"), a, b)
    tab = run("info", "-t", str(tmp_path / "both.msh")).stdout.splitlines()
    assert len(tab) == 1 + 6


def test_fastx_reader_has_kseq_semantics(built, tmp_path):
    lib = C.CDLL(os.path.join(ROOT, "tests", "libmshio.so"))
    lib.fastx_count.restype = C.c_long
    tb, nb = C.c_ulonglong(), C.c_ulonglong()
    n = lib.fastx_count(os.path.join(GOLD, "reads1.fastq.gz").encode(), C.c_long(0), C.byref(tb), C.byref(nb))
    recs = helpers.read_fastx(os.path.join(GOLD, "reads1.fastq.gz"))
    assert n == len(recs) == 1000 and tb.value == sum(len(r[2]) for r in recs)
    fa = tmp_path / "x.fa"
    fa.write_bytes(b"junk before\n>s1 first comment\r\nACGT\nAC GT\n\n>s2\nAAAA>s3 c\nTT\n>s4 tail")
    n = lib.fastx_count(str(fa).encode(), C.c_long(0), C.byref(tb), C.byref(nb))
    assert n == 4 and tb.value == 8 + 4 + 2 + 0                  # '>' mid-line starts a record, as in kseq
    fq = tmp_path / "bad.fq"
    fq.write_bytes(b"@r1\nACGT\n+\nII\n")
    assert lib.fastx_count(str(fq).encode(), C.c_long(0), C.byref(tb), C.byref(nb)) == -2


def _kseq_bytewise(data):
    """kseq_read of the reference's vendored kseq.h (:171-208), one byte at a time.
    Returns ([(name, comment, seq)], status) with status -1 (EOF) or -2 (short quality)."""
    pos, n = 0, len(data)
    recs, last = [], 0

    def getc():
        nonlocal pos
        if pos >= n:
            return -1
        pos += 1
        return data[pos - 1]

    isspace = lambda c: c in (9, 10, 11, 12, 13, 32)
    while True:
        if last == 0:
            c = getc()
            while c != -1 and c not in (62, 64):
                c = getc()
            if c == -1:
                return recs, -1
            last = c
        name, comment, seq = bytearray(), bytearray(), bytearray()
        c = getc()
        while c != -1 and not isspace(c):
            name.append(c); c = getc()
        if c == -1 and not name:
            return recs, -1
        if c != 10 and c != -1:
            c = getc()
            while c != -1 and c != 10:
                comment.append(c); c = getc()
        c = getc()
        while c != -1 and c not in (62, 43, 64):
            if 33 <= c <= 126:
                seq.append(c)
            c = getc()
        if c in (62, 64):
            last = c
        if c != 43:
            if c == -1:
                last = 0
            recs.append((bytes(name), bytes(comment), bytes(seq)))
            continue
        c = getc()
        while c != -1 and c != 10:
            c = getc()
        if c == -1:
            return recs, -2
        q = 0
        while True:                                  # kseq.h:201 reads a byte, THEN tests qual.l < seq.l
            c = getc()
            if c == -1 or q >= len(seq):
                break
            if 33 <= c <= 127:
                q += 1
        last = 0
        if q != len(seq):
            return recs, -2
        recs.append((bytes(name), bytes(comment), bytes(seq)))


def test_fastx_reader_matches_bytewise_kseq_on_random_input(built, tmp_path):
    """The buffered reader against the byte-by-byte state machine on byte soup: headers and
    '+' anywhere, blank / CR / control / high bytes, records across the 64 KiB refill boundary,
    truncated quality strings."""
    lib = C.CDLL(os.path.join(ROOT, "tests", "libmshio.so"))
    lib.fastx_dump.restype = C.c_long
    lib.fastx_dump.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_ulonglong)]
    rng = np.random.default_rng(99)
    alpha = np.frombuffer(b"ACGTNacgt\n\n\r >@+\t-\x00\xff\x7f!I~", dtype=np.uint8)
    weights = np.array([30, 30, 30, 30, 3, 2, 2, 2, 2, 8, 8, 1, 2, 0.4, 0.4, 0.4, 0.5, 0.5, 0.2, 0.2, 0.2, 1, 1, 1])
    weights = weights / weights.sum()
    for trial in range(40):
        size = int(rng.choice([50, 2000, 70000, 140000]))
        body = rng.choice(alpha, size=size, p=weights).tobytes()
        if trial % 4 == 1:                                   # quality string followed DIRECTLY by the next header (no newline):
            body = b"@a\nACGT\n+\nIIII@b\nGGCC\n+\nIIII>c\nTTTT\n" + body      # kseq swallows that header byte (kseq.h:201)
        if trial % 4 == 0:                                   # a well-formed long FASTQ record across the buffer edge
            seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=66000).tobytes()
            body = b"@r1 c\n" + seq + b"\n+\n" + b"I" * (66000 if trial % 8 else 65990) + b"\n" + body
        path = tmp_path / ("f%d" % trial)
        path.write_bytes(body)
        out, ln = C.c_char_p(), C.c_ulonglong()
        status = lib.fastx_dump(str(path).encode(), C.byref(out), C.byref(ln))
        got = C.string_at(out, ln.value)
        want_recs, want_status = _kseq_bytewise(body)
        want = b"".join(a + b"\t" + b + b"\t" + c + b"\n" for a, b, c in want_recs)
        assert status == want_status and got == want, trial


def test_fastx_reader_on_pipes(built, tmp_path):
    """Unseekable inputs -- a FIFO, as `<(zcat x.gz)` or /dev/stdin give -- carry plain or gzipped
    data and must yield the same records as the regular file: nothing may be read from the
    descriptor before zlib gets it (the first record used to be lost)."""
    import gzip
    import threading
    lib = C.CDLL(os.path.join(ROOT, "tests", "libmshio.so"))
    lib.fastx_dump.restype = C.c_long
    lib.fastx_dump.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_ulonglong)]
    body = b">a first\nACGTACGTAA\nCCGG\n>b\nTTTTGGGG\n@c q\nACGT\n+\nIIII\n"

    def dump(path):
        out, ln = C.c_char_p(), C.c_ulonglong()
        status = lib.fastx_dump(str(path).encode(), C.byref(out), C.byref(ln))
        return status, C.string_at(out, ln.value)

    plain = tmp_path / "x.fa"
    plain.write_bytes(body)
    want = dump(plain)
    assert want[1].count(b"\n") == 3
    gz = tmp_path / "x.fa.gz"
    gz.write_bytes(gzip.compress(body))
    assert dump(gz) == want
    for payload in (body, gzip.compress(body)):
        fifo = tmp_path / "pipe"
        os.mkfifo(fifo)
        t = threading.Thread(target=lambda: open(fifo, "wb").write(payload))
        t.start()
        got = dump(fifo)
        t.join()
        os.unlink(fifo)
        assert got == want


# ---------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_make_test_recipe_on_gpu(built, tmp_path, oracle):
    """The reference's `make test` (Makefile.in:94-111) with what the mount provides:
    sketch reads -> info -d == reads.json (hashes/name/length/comment); dist == genomes.dist."""
    for f in ("reads1.fastq", "reads2.fastq"):
        with gzip.open(os.path.join(GOLD, f + ".gz"), "rb") as fi, open(tmp_path / f, "wb") as fo:
            shutil.copyfileobj(fi, fo)
    r = run("sketch", "-r", "-I", "reads", "reads1.fastq", "reads2.fastq", "-o", "reads.msh", cwd=tmp_path)
    assert "Writing to reads.msh..." in r.stderr
    dump = run("info", "-d", "reads.msh", cwd=tmp_path).stdout
    # -r implies -M (sketchParameterSetup.cpp:62-65): the current reference code also dumps a
    # "counts" array (CommandInfo.cpp:265-283); the golden reads.json predates that,
    # so compare with the counts block removed, and check the counts against the oracle.
    a, b = dump.index('\t\t\t"counts" :'), dump.index("\t\t}\n\t]")
    counts = [int(x.strip().rstrip(",")) for x in dump[a:b].splitlines()[2:-1]]
    assert dump[:a] + dump[b:] == open(os.path.join(GOLD, "reads.json")).read()
    recs = [r[2] for r in helpers.round_robin([helpers.read_fastx(str(tmp_path / "reads1.fastq")),
                                               helpers.read_fastx(str(tmp_path / "reads2.fastq"))])]
    _, oc, _, _, _ = oracle.sketch_records(recs, oracle.params(k=21, s=1000))
    assert counts == [int(x) for x in oc]
    # -m 2: a hash enters the sketch at its second occurrence (MinHashHeap.cpp:96-118)
    r2 = run("sketch", "-r", "-m", "2", "-o", "reads_m2", "reads1.fastq", "reads2.fastq", cwd=tmp_path)
    dump2 = run("info", "-d", "reads_m2.msh", cwd=tmp_path).stdout       # (the reference's dump with counts is not strict JSON)
    ha, hb = dump2.index('\t\t\t"hashes" :'), dump2.index('\t\t\t"counts" :')
    hashes2 = [int(x.strip().rstrip(",")) for x in dump2[ha:hb].splitlines()[2:] if x.strip().rstrip(",").isdigit()]
    counts2 = [int(x.strip().rstrip(",")) for x in dump2[hb:dump2.index("\t\t}\n\t]")].splitlines()[2:-1]]
    oh, oc2, _, osz, _ = oracle.sketch_records(recs, oracle.params(k=21, s=1000, min_copies=2))
    assert hashes2 == [int(x) for x in oh] and counts2 == [int(x) for x in oc2]
    assert '"length" : %d,' % int(osz) in dump2 and min(counts2) >= 2 and "Estimated coverage:" in r2.stderr
    # -c 3: reading stops once the average multiplicity of the kept hashes reaches 3 (Sketch.cpp:1258)
    r3 = run("sketch", "-r", "-c", "3", "-o", "reads_c3", "reads1.fastq", "reads2.fastq", cwd=tmp_path)
    oh3, oc3, osz3, oused3, omult3 = oracle.sketch_reads(recs, oracle.params(k=21, s=1000, target_cov=3.0))
    dump3 = run("info", "-d", "reads_c3.msh", cwd=tmp_path).stdout
    ha, hb = dump3.index('\t\t\t"hashes" :'), dump3.index('\t\t\t"counts" :')
    hashes3 = [int(x.strip().rstrip(",")) for x in dump3[ha:hb].splitlines()[2:] if x.strip().rstrip(",").isdigit()]
    assert hashes3 == [int(x) for x in oh3]
    assert "Reads used:            %d" % oused3 in r3.stderr and '"comment" : "[%d seqs] ' % oused3 in dump3
    assert "Estimated coverage:    %s" % helpers.fmt_g(omult3) in r3.stderr
    bad = run("sketch", "-r", "-m", "2", "-b", "1G", "-o", "x", "reads1.fastq", cwd=tmp_path, check=False)
    assert bad.returncode == 1 and "cannot be used with" in bad.stderr
    # -b: Bloom filter in front of the heap (MinHashHeap.cpp:78-94), on the reference's own test reads,
    # filter sizes from aliasing (3K) to none (8M); -b implies -r; the read chunk size does not matter
    for bb, nbytes in (("3K", 3000), ("8M", 8000000)):
        rb = run("sketch", "-b", bb, "-o", "reads_b" + bb, "reads1.fastq", "reads2.fastq", cwd=tmp_path)
        ohb, ocb, _, oszb, omultb = oracle.sketch_records(recs, oracle.params(k=21, s=1000, bloom_bytes=nbytes))
        dumpb = run("info", "-d", "reads_b%s.msh" % bb, cwd=tmp_path).stdout
        ha, hb = dumpb.index('\t\t\t"hashes" :'), dumpb.index('\t\t\t"counts" :')
        hashesb = [int(x.strip().rstrip(",")) for x in dumpb[ha:hb].splitlines()[2:] if x.strip().rstrip(",").isdigit()]
        countsb = [int(x.strip().rstrip(",")) for x in dumpb[hb:dumpb.index("\t\t}\n\t]")].splitlines()[2:-1]]
        assert hashesb == [int(x) for x in ohb] and countsb == [int(x) for x in ocb], bb
        assert '"length" : %d,' % int(oszb) in dumpb and min(countsb) >= 2
        env = dict(os.environ, MASH_AMD_READS_CHUNK="20000")
        run("sketch", "-b", bb, "-o", "reads_bc" + bb, "reads1.fastq", "reads2.fastq", cwd=tmp_path, env=env)
        assert run("info", "-d", "reads_bc%s.msh" % bb, cwd=tmp_path).stdout == dumpb
    # reads options reach every query file of dist / triangle (initFromFiles -> sketchFile, Sketch.cpp:1156):
    # the two estimate lines per file, and a file of which nothing is kept (-m 2 on a sequence without
    # repeated k-mers) ends the run like an empty file (reference.length == 0, Sketch.cpp:1302-1314)
    rng = np.random.default_rng(77)
    with open(tmp_path / "uniq.fa", "wb") as f:
        f.write(b">u\n" + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 5000)].tobytes() + b"\n")
    rq = run("dist", "-r", "reads.msh", "reads1.fastq", "uniq.fa", cwd=tmp_path)
    assert rq.stderr.count("Estimated genome size:") == 2 and rq.stderr.count("Estimated coverage:") == 2
    assert len(rq.stdout.splitlines()) == 2
    empty = run("dist", "-m", "2", "reads.msh", "reads1.fastq", "uniq.fa", cwd=tmp_path, check=False)
    assert empty.returncode == 1 and 'ERROR: Did not find fasta records in "input files".' in empty.stderr
    assert empty.stderr.count("Estimated genome size:") == 1                  # reads1.fastq was sketched before the refusal
    # a reference SKETCH fixes the sketch size of a reads-mode query (CommandDistance.cpp:121-128)
    mism = run("dist", "-s", "300", "-r", "reads.msh", "reads1.fastq", cwd=tmp_path, check=False)
    assert mism.returncode == 1 and mism.stdout == "" and "ERROR: The sketch size must match the reference when using a bloom filter" in mism.stderr
    assert run("dist", "-s", "1000", "-r", "reads.msh", "reads1.fastq", cwd=tmp_path).stdout == rq.stdout.splitlines(True)[0]
    hist = run("info", "-c", "reads.msh", cwd=tmp_path).stdout.splitlines()
    assert hist[0] == "#Sketch\tBin\tFrequency" and sum(int(l.split("\t")[2]) for l in hist[1:]) == 1000
    assert "Estimated coverage:" in r.stderr
    run("json2msh", os.path.join(GOLD, "genomes.json"), "genomes.msh", cwd=tmp_path)
    out = run("dist", "genomes.msh", "reads.msh", cwd=tmp_path).stdout
    assert out == open(os.path.join(GOLD, "genomes.dist")).read()
    # gz input, table output, filters
    out_t = run("dist", "-t", "genomes.msh", "reads.msh", cwd=tmp_path).stdout.splitlines()
    assert out_t[0] == "#query\tgenome1.fna\tgenome2.fna\tgenome3.fna" and out_t[1] == "reads\t0.12101\t0.12827\t0.12101"
    out_d = run("dist", "-d", "0.125", "genomes.msh", "reads.msh", cwd=tmp_path).stdout.splitlines()
    assert len(out_d) == 2 and all("0.12101" in l for l in out_d)


@pytest.mark.gpu
def test_min_copies_zero_keeps_nothing_like_the_reference(built, tmp_path):
    """-m 0: `multiplicityMinimum - 1` wraps in the reference's heap (MinHashHeap.cpp:96-118, uint64_t),
    no pending count ever equals it and nothing is admitted: the sketch is empty, which sketchFile
    refuses (Sketch.cpp:1302-1314) unless -g supplies a length.  Same text, same exit status; with -g
    the three m0_* fixtures of the reference CLI compare the written sketch."""
    import gzip, shutil
    with gzip.open(os.path.join(GOLD, "reads1.fastq.gz"), "rb") as fi, open(tmp_path / "r.fq", "wb") as fo:
        shutil.copyfileobj(fi, fo)
    ours = subprocess.run([MASH, "sketch", "-m", "0", "-o", "x", "r.fq"], cwd=tmp_path, capture_output=True)
    assert ours.returncode == 1 and not (tmp_path / "x.msh").exists()
    assert ours.stderr.decode().strip().splitlines()[-1] == 'ERROR: Did not find fasta records in "input files".'
    ref = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
    if os.path.exists(ref):
        theirs = subprocess.run([ref, "sketch", "-m", "0", "-o", "y", "r.fq"], cwd=tmp_path, capture_output=True)
        assert (theirs.returncode, theirs.stderr) == (ours.returncode, ours.stderr)
        for extra in (["-g", "12345"], ["-g", "777", "-c", "3"]):
            a = subprocess.run([MASH, "sketch", "-m", "0", *extra, "-o", "x", "r.fq"], cwd=tmp_path, capture_output=True)
            b = subprocess.run([ref, "sketch", "-m", "0", *extra, "-o", "y", "r.fq"], cwd=tmp_path, capture_output=True)
            assert (a.returncode, a.stderr.replace(b"x.msh", b"y.msh")) == (b.returncode, b.stderr)
            assert (tmp_path / "x.msh").read_bytes() == (tmp_path / "y.msh").read_bytes()


@pytest.mark.gpu
def test_make_test_screen_recipe_on_gpu(built, tmp_path):
    """testScreen of the reference's Makefile (Makefile.in:113-115):
    mash screen genomes.msh reads1.fastq reads2.fastq == test/ref/screen, byte for byte."""
    for f in ("reads1.fastq", "reads2.fastq"):
        with gzip.open(os.path.join(GOLD, f + ".gz"), "rb") as fi, open(tmp_path / f, "wb") as fo:
            shutil.copyfileobj(fi, fo)
    run("json2msh", os.path.join(GOLD, "genomes.json"), "genomes.msh", cwd=tmp_path)
    r = run("screen", "genomes.msh", "reads1.fastq", "reads2.fastq", cwd=tmp_path)
    assert r.stdout == open(os.path.join(GOLD, "screen")).read()
    assert "Estimated distinct k-mers in mixture: 502359" in r.stderr and "distinct hashes." in r.stderr
    w = run("screen", "-w", "genomes.msh", "reads1.fastq", "reads2.fastq", cwd=tmp_path).stdout.splitlines()
    tot = sum(int(l.split("\t")[1].split("/")[0]) for l in w)
    assert 44 <= tot <= 44 + 36 and len(w) >= 1                      # shared hashes are assigned to one winner each
    none = run("screen", "-i", "0.95", "genomes.msh", "reads1.fastq", cwd=tmp_path).stdout
    assert none == ""
    # several GPUs (two contexts on device 0 here) and many small batches: the mixture is sharded by
    # batch (mg_dscreen), the counters are summed -- same bytes on stdout and stderr
    multi = run("screen", "genomes.msh", "reads1.fastq", "reads2.fastq", cwd=tmp_path,
                env={"MASH_GPU_DEVICES": "0,0", "MASH_AMD_SCREEN_BATCH": "40000"})
    assert multi.stdout == r.stdout and multi.stderr == r.stderr


@pytest.mark.gpu
def test_screen_protein_queries_translate_the_mixture(built, tmp_path, oracle):
    """`mash screen` with amino-acid sketches (`mash sketch -a`): the nucleotide mixture is
    6-frame translated (CommandScreen.cpp:120, 516-531); shared counts vs the oracle."""
    rng = np.random.default_rng(17)
    k, s = 9, 200
    genomes = [synth._rand_dna(rng, 6000) for _ in range(2)]
    with open(tmp_path / "prot.faa", "wb") as f:
        for i, g in enumerate(genomes):
            for j, fr in enumerate(oracle.six_frames(g)):
                f.write(b">g%d_f%d\n%s\n" % (i, j, fr.replace(b"*", b"X")))    # X is outside the alphabet too
    # one sketch per genome: six records each
    for i in range(2):
        with open(tmp_path / ("p%d.faa" % i), "wb") as f:
            for j, fr in enumerate(oracle.six_frames(genomes[i])):
                f.write(b">g%d_f%d\n%s\n" % (i, j, fr.replace(b"*", b"X")))
    run("sketch", "-a", "-k", str(k), "-s", str(s), "-o", "prot", "p0.faa", "p1.faa", cwd=tmp_path)
    reads = []
    with open(tmp_path / "mix.fa", "wb") as f:
        for n in range(600):
            l = int(rng.integers(60, 150))
            st = int(rng.integers(0, 6000 - l))
            r = genomes[0][st:st + l]                                  # only genome 0 is in the mixture
            reads.append(r)
            f.write(b">r%d\n%s\n" % (n, r))
    only_hits = run("screen", "prot.msh", "mix.fa", cwd=tmp_path).stdout.splitlines()
    out = run("screen", "-i", "-1", "prot.msh", "mix.fa", cwd=tmp_path)      # -1: also queries sharing nothing
    assert "Translating from mix.fa..." in out.stderr and "(translated)" in out.stderr
    prot = "ACDEFGHIKLMNPQRSTVWY"
    want = set()
    for r in reads:
        for fr in oracle.six_frames(r):
            if len(fr) >= k:
                want.update(int(x) for x in oracle.sketch_records([fr], oracle.params(k=k, s=10 ** 6, alphabet=prot, noncanonical=True))[0])
    lines = [l.split("\t") for l in out.stdout.splitlines()]
    assert [l[4] for l in lines] == ["p0.faa", "p1.faa"]
    for i, l in enumerate(lines):
        recs = [fr.replace(b"*", b"X") for fr in oracle.six_frames(genomes[i])]
        sk = oracle.sketch_records(recs, oracle.params(k=k, s=s, alphabet=prot, noncanonical=True))[0]
        shared = sum(1 for x in sk if int(x) in want)
        assert l[1] == "%d/%d" % (shared, s), (i, l)
        ident = 1.0 if shared == s else (0.0 if shared == 0 else (shared / s) ** (1.0 / k))
        assert l[0] == helpers.fmt_g(ident)
    assert int(lines[0][1].split("/")[0]) > 100 > int(lines[1][1].split("/")[0])
    assert [l.split("\t")[4] for l in only_hits] == [l[4] for l in lines if not l[1].startswith("0/")]


@pytest.mark.gpu
def test_sketch_and_triangle_cli_vs_oracle(built, tmp_path, oracle):
    rng = np.random.default_rng(3)
    genomes = [synth._rand_dna(rng, 40000) for _ in range(5)]
    genomes[1] = genomes[0][:20000] + genomes[1][20000:]              # related pair
    genomes[4] = genomes[0]                                           # identical pair
    fa = tmp_path / "multi.fa"
    with open(fa, "wb") as f:
        for i, g in enumerate(genomes):
            f.write(b">seq%d comment %d\n" % (i, i))
            for o in range(0, len(g), 70):
                f.write(g[o:o + 70] + b"\n")
        f.write(b">tiny\nACGT\n")
    # -i : one sketch per record (records < k skipped)
    run("sketch", "-i", "-s", "400", "-o", "ind", "multi.fa", cwd=tmp_path)
    tab = run("info", "-t", "ind.msh", cwd=tmp_path).stdout.splitlines()[1:]
    assert [l.split("\t")[2] for l in tab] == ["seq%d" % i for i in range(5)]
    assert [l.split("\t")[1] for l in tab] == ["40000"] * 5
    p = oracle.params(k=21, s=400)
    import json
    dump = json.loads(run("info", "-d", "ind.msh", cwd=tmp_path).stdout)
    for i, g in enumerate(genomes):
        h, _, _, _, _ = oracle.sketch_records([g], p)
        assert dump["sketches"][i]["hashes"] == [int(x) for x in h]
        assert dump["sketches"][i]["comment"] == "comment %d" % i
    # concatenated default: one sketch, comment "[5 seqs] seq0 comment 0 [...]", length = sum of records >= k
    run("sketch", "-s", "400", "-o", "cat", "multi.fa", cwd=tmp_path)
    t = run("info", "-t", "cat.msh", cwd=tmp_path).stdout.splitlines()[1].split("\t")
    assert t[1] == "200000" and t[2] == "multi.fa" and t[3] == "[5 seqs] seq0 comment 0 [...]"
    # triangle on the single multi-fasta (=> per-sequence sketches, CommandTriangle.cpp:74-77)
    r = run("triangle", "-s", "400", "multi.fa", cwd=tmp_path)
    lines = r.stdout.splitlines()
    assert lines[0] == "\t5" and lines[1] == "seq0"
    kspace = 4.0 ** 21
    sk = [oracle.sketch_records([g], p)[0] for g in genomes]
    for i in range(1, 5):
        f = lines[1 + i].split("\t")
        assert f[0] == "seq%d" % i and len(f) == i + 1
        for j in range(i):
            o = oracle.compare(sk[i], sk[j], 40000, 40000, 400, 21, kspace)
            assert f[1 + j] == "%g" % o.distance
    assert "Max p-value:" in r.stderr
    assert lines[5].split("\t")[1] == "0"                            # identical pair
    # edge list agrees with dist on the same sketches
    e = run("triangle", "-E", "ind.msh", cwd=tmp_path).stdout.splitlines()
    d = run("dist", "ind.msh", "ind.msh", cwd=tmp_path).stdout.splitlines()
    dd = {(l.split("\t")[0], l.split("\t")[1]): l.split("\t")[2:] for l in d}
    assert len(e) == 10
    for l in e:
        a, b, *rest = l.split("\t")
        assert dd[(b, a)] == rest
    # thresholded runs: the device-side filter path and the full path print the same lines
    nofilter = {"MASH_AMD_NO_FILTER": "1"}
    for d_max in ("0", "0.05", "0.2", "0.9"):
        for cmd in (("triangle", "-E", "-d", d_max, "ind.msh"), ("dist", "-d", d_max, "ind.msh", "ind.msh"),
                    ("dist", "-d", d_max, "-v", "1e-10", "ind.msh", "cat.msh")):
            a = run(*cmd, cwd=tmp_path).stdout
            b = run(*cmd, cwd=tmp_path, env=nofilter).stdout
            assert a == b, cmd
    # the device tail (distance table + exact p-value + both filters, finish.hip) prints what the host tail prints
    hostfin = {"MASH_AMD_HOST_FINISH": "1"}
    for cmd in (("triangle", "-E", "ind.msh"), ("triangle", "-E", "-v", "1e-5", "ind.msh"), ("triangle", "-E", "-d", "0.1", "-v", "1e-20", "ind.msh"),
                ("dist", "ind.msh", "cat.msh"), ("dist", "-v", "1e-8", "ind.msh", "ind.msh"), ("dist", "-d", "0.3", "-v", "1e-3", "ind.msh", "cat.msh"),
                ("dist", "-t", "-v", "1e-8", "ind.msh", "ind.msh")):
        a = run(*cmd, cwd=tmp_path).stdout
        b = run(*cmd, cwd=tmp_path, env=hostfin).stdout
        assert a == b and (a or "-v" in cmd), cmd
    # several GPUs (here: two contexts on device 0): rows sharded by mg_compare_*_sharded_host, same bytes
    two = {"MASH_GPU_DEVICES": "0,0"}
    for cmd in (("triangle", "ind.msh"), ("triangle", "-E", "ind.msh"), ("triangle", "-E", "-d", "0.2", "ind.msh"),
                ("dist", "ind.msh", "cat.msh"), ("dist", "-t", "ind.msh", "ind.msh"), ("dist", "-d", "0.3", "-v", "1e-3", "ind.msh", "cat.msh")):
        a = run(*cmd, cwd=tmp_path)
        b = run(*cmd, cwd=tmp_path, env=two)
        assert a.stdout == b.stdout and a.stderr == b.stderr, cmd
    e0 = run("triangle", "-d", "0", "ind.msh", cwd=tmp_path).stdout.splitlines()
    assert len(e0) == 1 and e0[0].split("\t")[:3] == ["seq4", "seq0", "0"]


@pytest.mark.gpu
def test_many_short_records_are_sketched_in_bounded_batches(built, tmp_path):
    """`-i` over a file of many short records: batches are flushed by hash slots (sketches x
    sketch size), not only by bytes, so memory stays bounded -- and the .msh does not depend on
    where the batches end (MASH_AMD_BATCH_HASHES forces a flush every few sketches)."""
    rng = np.random.default_rng(5)
    recs = [b">r%d amplicon\n" % i + np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 600)].tobytes() + b"\n"
            for i in range(300)]
    fa = tmp_path / "amp.fa"
    fa.write_bytes(b"".join(recs))
    run("sketch", "-i", "-s", "500", "-o", str(tmp_path / "one"), str(fa))
    run("sketch", "-i", "-s", "500", "-o", str(tmp_path / "many"), str(fa), env={"MASH_AMD_BATCH_HASHES": "3500"})
    assert (tmp_path / "one.msh").read_bytes() == (tmp_path / "many.msh").read_bytes()
    # concatenated mode over many small files takes the same cap
    files = []
    for i in range(12):
        f = tmp_path / f"g{i}.fa"
        f.write_bytes(recs[i])
        files.append(str(f))
    run("sketch", "-s", "500", "-o", str(tmp_path / "c1"), *files)
    run("sketch", "-s", "500", "-o", str(tmp_path / "c2"), *files, env={"MASH_AMD_BATCH_HASHES": "1200"})
    assert (tmp_path / "c1.msh").read_bytes() == (tmp_path / "c2.msh").read_bytes()
    # streamed ingest (segments -> pinned ring -> device while parsing) vs the concatenate-then-copy path
    for extra in ((), ("-p", "4"), ("-i",), ("-M",), ("-r",), ("-r", "-m", "2")):
        run("sketch", "-s", "500", *extra, "-o", str(tmp_path / "s1"), *files, str(fa))
        run("sketch", "-s", "500", *extra, "-o", str(tmp_path / "s2"), *files, str(fa), env={"MASH_AMD_NO_STREAM": "1"})
        run("sketch", "-s", "500", *extra, "-o", str(tmp_path / "s3"), *files, str(fa), env={"MASHGPU_STAGE_BYTES": "333"})
        assert (tmp_path / "s1.msh").read_bytes() == (tmp_path / "s2.msh").read_bytes() == (tmp_path / "s3.msh").read_bytes(), extra
    # -c: the reads session is fed chunk by chunk and reading stops with the chunk that reaches the
    # coverage; same sketch and same "Reads used" whatever the chunk size
    reads = tmp_path / "cov.fa"
    reads.write_bytes(b"".join(recs[i % 40] for i in range(400)))
    a = run("sketch", "-r", "-c", "3", "-s", "200", "-o", str(tmp_path / "v1"), str(reads))
    b = run("sketch", "-r", "-c", "3", "-s", "200", "-o", str(tmp_path / "v2"), str(reads), env={"MASH_AMD_READS_CHUNK": "3000"})
    assert (tmp_path / "v1.msh").read_bytes() == (tmp_path / "v2.msh").read_bytes()
    used = [l for l in a.stderr.splitlines() if l.startswith("Reads used:")]
    assert used and used == [l for l in b.stderr.splitlines() if l.startswith("Reads used:")]
    assert int(used[0].split()[-1]) < 400                                    # stopped before the end of the input
    # plain -r / -m in constant memory (the default since round 3: a reads session, chunk by chunk) against the
    # route that keeps the whole read set in HBM for one sketch call: same .msh whatever the chunk size -- incl.
    # the multiplicities (-M is implied by -r) and with them the order-dependent count of the largest kept hash
    for extra in (("-r",), ("-r", "-m", "2"), ("-r", "-m", "3", "-k", "15")):
        run("sketch", *extra, "-s", "200", "-o", str(tmp_path / "m1"), str(reads))
        run("sketch", *extra, "-s", "200", "-o", str(tmp_path / "m2"), str(reads), env={"MASH_AMD_READS_CHUNK": "3000"})
        run("sketch", *extra, "-s", "200", "-o", str(tmp_path / "m3"), str(reads), env={"MASH_AMD_READS_RESIDENT": "1"})
        assert (tmp_path / "m1.msh").read_bytes() == (tmp_path / "m2.msh").read_bytes() == (tmp_path / "m3.msh").read_bytes(), extra


@pytest.mark.gpu
def test_parallel_ingest_keeps_input_order(built, tmp_path):
    """-p N parses files on worker threads; sketches come out in input order, byte-identical
    to the single-threaded run (ThreadPool delivers in submission order, ThreadPool.hxx:127-167)."""
    rng = np.random.default_rng(23)
    names = []
    for i in range(9):
        n = "g%d.fa" % i
        names.append(n)
        with open(tmp_path / n, "wb") as f:
            for r in range(int(rng.integers(1, 4))):
                f.write(b">c%d_%d some comment\n%s\n" % (i, r, synth._rand_dna(rng, int(rng.integers(2000, 30000)))))
    run("sketch", "-s", "200", "-o", "seq", *names, cwd=tmp_path)
    run("sketch", "-p", "4", "-s", "200", "-o", "par", *names, cwd=tmp_path)
    assert open(tmp_path / "seq.msh", "rb").read() == open(tmp_path / "par.msh", "rb").read()
    tab = run("info", "-t", "par.msh", cwd=tmp_path).stdout.splitlines()[1:]
    assert [l.split("\t")[2] for l in tab] == names
    missing = run("sketch", "-p", "4", "-o", "x", names[0], "nope.fa", names[1], cwd=tmp_path, check=False)
    assert missing.returncode == 1 and "could not open nope.fa" in missing.stderr



@pytest.mark.gpu
def test_large_outputs_do_not_depend_on_formatting_threads(built, tmp_path):
    """Blocks of result rows are formatted on worker threads (mash_main.cpp::emit_rows) and
    finished on host threads inside the library; the text must equal the one-thread run."""
    rng = np.random.default_rng(31)
    base = np.frombuffer(synth._rand_dna(rng, 3000), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(tmp_path / "many.fa", "wb") as f:
        for i in range(1000):
            seq = base.copy()
            idx = rng.integers(0, 3000, int(rng.integers(0, 600)))
            seq[idx] = lut[rng.integers(0, 4, len(idx))]
            f.write(b">r%d c%d\n%s\n" % (i, i, seq.tobytes()))
    run("sketch", "-i", "-s", "64", "-k", "15", "-o", "many", "many.fa", cwd=tmp_path)
    one = {"MASH_AMD_EMIT_THREADS": "1"}
    many = {"MASH_AMD_EMIT_THREADS": "7"}
    for cmd in (("triangle", "many.msh"), ("triangle", "-E", "many.msh"), ("triangle", "-C", "-v", "1e-5", "many.msh"),
                ("dist", "many.msh", "many.msh"), ("dist", "-t", "many.msh", "many.msh"),
                ("dist", "-v", "1e-8", "-C", "many.msh", "many.msh")):
        a = run(*cmd, cwd=tmp_path, env=one)
        b = run(*cmd, cwd=tmp_path, env=many)
        assert a.stdout == b.stdout and a.stderr == b.stderr, cmd
        assert len(a.stdout) > 1000
    # the Phylip path takes distances from a table and skips p-values that cannot raise the peak:
    # same matrix and same "Max p-value" as finishing every pair
    a = run("triangle", "many.msh", cwd=tmp_path)
    b = run("triangle", "many.msh", cwd=tmp_path, env={"MASH_AMD_FULL_FINISH": "1"})
    assert a.stdout == b.stdout and a.stderr == b.stderr and "Max p-value:" in a.stderr
    for cmd in (("dist", "-t", "many.msh", "many.msh"), ("dist", "-t", "-d", "0.08", "many.msh", "many.msh")):
        a = run(*cmd, cwd=tmp_path)
        b = run(*cmd, cwd=tmp_path, env={"MASH_AMD_FULL_FINISH": "1"})
        assert a.stdout == b.stdout, cmd
    tri = run("triangle", "many.msh", cwd=tmp_path, env=many).stdout.splitlines()
    assert tri[0] == "\t1000" and len(tri) == 1001
    assert [len(l.split("\t")) for l in tri[1:]] == list(range(1, 1001))
    d = run("dist", "many.msh", "many.msh", cwd=tmp_path, env=many).stdout.splitlines()
    assert len(d) == 1000 * 1000
    assert d[1000 * 7 + 3].split("\t")[:2] == ["r3", "r7"]


@pytest.mark.gpu
def test_outputs_do_not_depend_on_block_boundaries(built, tmp_path):
    """The compare commands work through their rows in blocks of a pair budget per route (mash_main.cpp::Blocks) and carry
    state over them: the running "Max p-value", the offset of a block in the triangle, the exceptions of a row, the query
    lengths of a block.  MASH_AMD_BLOCK_PAIRS lowers every budget: 1000 gives blocks of several rows, 1 one row per block
    (a block always takes its first row).  stdout, stderr and exit status must equal the run with the default budgets,
    which this table (299 sketches, 44 551 pairs) fits into as one block.
    The input: 300 records, mutated copies of one 3 kb base as in the test above; one of them is shorter than k, which
    `sketch -i` drops as the reference does, and one has no valid k-mer: that one is the empty sketch of the table."""
    rng = np.random.default_rng(37)
    base = np.frombuffer(synth._rand_dna(rng, 3000), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(tmp_path / "many.fa", "wb") as f:
        for i in range(300):
            seq = base.copy()
            idx = rng.integers(0, 3000, int(rng.integers(0, 600)))
            seq[idx] = lut[rng.integers(0, 4, len(idx))]
            text = seq.tobytes()
            if i == 120:
                text = text[:9]                                    # shorter than k
            if i == 211:
                text = b"N" * 100                                  # no k-mer to hash
            f.write(b">r%d c%d\n%s\n" % (i, i, text))
    run("sketch", "-i", "-s", "64", "-k", "15", "-o", "many", "many.fa", cwd=tmp_path)
    nhashes = [l.split("\t")[0] for l in run("info", "-t", "many.msh", cwd=tmp_path).stdout.splitlines()[1:]]
    assert len(nhashes) == 299 and nhashes.count("0") == 1
    one, two = ("many.msh",), ("many.msh", "many.msh")
    host, nofilter = {"MASH_AMD_HOST_FINISH": "1"}, {"MASH_AMD_NO_FILTER": "1"}
    tri_edges, tri_near = ("triangle", "-E", "-d", "0.1", "-v", "1e-5") + one, ("triangle", "-N", "3", "-d", "0.2") + one
    dist_cut, dist_near, dist_tab_cut = ("dist", "-d", "0.1") + two, ("dist", "-N", "3") + two, ("dist", "-t", "-v", "1e-8") + two
    cluster = ("cluster", "-d", "0.05") + one
    cases = [(("triangle",) + one, {}), (("triangle",) + one, {"MASH_AMD_DENSE_MATRIX": "1"}), (("triangle",) + one, {"MASH_AMD_FULL_FINISH": "1"}),
             (("triangle", "-E") + one, {}), (tri_edges, {}), (tri_near, {}),
             (("dist",) + two, {}), (("dist", "-t") + two, {}), (dist_tab_cut, {}), (dist_cut, {}), (dist_near, {}), (cluster, {}),
             (tri_edges, host), (tri_near, host), (dist_tab_cut, host), (dist_cut, host), (dist_near, host), (cluster, host),
             (tri_edges, nofilter), (dist_cut, nofilter)]
    plain = {}
    for cmd, env in cases:
        a = run(*cmd, cwd=tmp_path, env=env)
        assert len(a.stdout) > 0, (cmd, env)
        if not env:
            plain[cmd] = a.stdout
        for budget in ("1000", "1"):
            b = run(*cmd, cwd=tmp_path, env=dict(env, MASH_AMD_BLOCK_PAIRS=budget), check=False)
            assert (b.returncode, b.stdout, b.stderr) == (a.returncode, a.stdout, a.stderr), (cmd, env, budget)
        if cmd[0] == "triangle" and "-E" not in cmd and "-N" not in cmd:
            assert "Max p-value:" in a.stderr
    # the filters cut somewhere in the middle, or the thresholded routes above were vacuous
    nlines = {cmd: out.count("\n") for cmd, out in plain.items()}
    assert 0 < nlines[tri_edges] < nlines[("triangle", "-E") + one]
    assert 0 < nlines[tri_near] < nlines[("triangle", "-E") + one]
    assert 0 < nlines[dist_cut] < nlines[("dist",) + two]
    assert 0 < nlines[dist_near] <= 3 * 299 < nlines[("dist",) + two]
    cells = lambda out: sum(1 for l in out.splitlines()[1:] for c in l.split("\t")[1:] if c)
    assert 0 < cells(plain[dist_tab_cut]) < cells(plain[("dist", "-t") + two])
    assert 1 < max(int(l.split("\t")[0]) for l in plain[cluster].splitlines()) < 299      # neither one cluster nor all singletons


def test_msh_reader_survives_corrupted_files(built, tmp_path):
    """Truncated or bit-flipped .msh files (wrong segment table, pointers past the end, absurd
    list lengths) must end in an error message and exit status 1, never in a crash."""
    import random
    msh = str(tmp_path / "g.msh")
    run("json2msh", os.path.join(GOLD, "genomes.json"), msh)
    data = open(msh, "rb").read()
    rnd = random.Random(7)
    bad = str(tmp_path / "bad.msh")
    outcomes = set()
    for it in range(120):
        b = bytearray(data)
        mode = rnd.random()
        if mode < 0.3:
            b = b[: rnd.randrange(0, len(b))]
        elif mode < 0.8:
            for _ in range(rnd.randrange(1, 8)):
                i = rnd.randrange(0, 4096 if rnd.random() < 0.7 else len(b))
                b[i] = rnd.randrange(256)
        else:
            i = rnd.randrange(0, len(b) - 8)
            b[i:i + 8] = bytes(rnd.randrange(256) for _ in range(8))
        open(bad, "wb").write(b)
        for args in (("info", "-d", bad), ("info", "-t", bad)):
            r = subprocess.run([MASH, *args], capture_output=True)      # bytes: corrupted names are not UTF-8
            assert r.returncode in (0, 1), (it, args, r.returncode, r.stderr[-200:])
            outcomes.add(r.returncode)
    assert 1 in outcomes


def test_info_and_paste_behave_like_the_reference_cli(built, tmp_path):
    """`mash info` / `mash paste` need no GPU, so where the reference CLI has been built
    (oracle/_ref/mash-ref, make -C oracle refcli) both binaries are run side by side on sketches
    written by the reference's code: same stdout, same stderr, same exit status -- including the
    refusals (incompatible options, missing or non-sketch inputs, mismatched k-mer sizes, existing
    output)."""
    ref = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
    cli_in = os.path.join(GOLD, "cli", "in")
    if not os.path.exists(ref):
        pytest.skip("reference CLI not built here (make -C oracle refcli)")
    dirs = {}
    for tag, exe in (("ref", ref), ("ours", MASH)):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(cli_in):
            shutil.copy(os.path.join(cli_in, f), d)
        # the sketches always come from the reference's code (ours would need the GPU)
        for args in (["sketch", "-s", "300", "-o", "a", "g1.fa", "g2.fa", "g3.fa"], ["sketch", "-M", "-s", "100", "-o", "m", "g1.fa", "g3.fa"],
                     ["sketch", "-k", "16", "-s", "120", "-i", "-o", "b", "multi.fa"], ["sketch", "-a", "-k", "9", "-s", "150", "-i", "-o", "p", "prot.fa"],
                     ["sketch", "-s", "300", "-o", "d", "g4.fa"], ["sketch", "-S", "9", "-s", "300", "-o", "s9", "g4.fa"]):
            subprocess.run([ref, *args], cwd=d, capture_output=True, check=True)
        open(d / "mshlist.txt", "w").write("a.msh\nd.msh\n")
        dirs[tag] = (exe, d)
    cases = [["info", "-t", "a.msh"], ["info", "-H", "a.msh"], ["info", "-d", "b.msh"], ["info", "-d", "m.msh"], ["info", "-c", "m.msh"],
             ["info", "-c", "a.msh"], ["info", "-t", "p.msh"], ["info", "-H", "p.msh"], ["info", "-d", "p.msh"], ["info", "-H", "m.msh"],
             ["info", "-H", "s9.msh"], ["info", "-H", "-t", "a.msh"], ["info", "-d", "-c", "a.msh"], ["info", "-t", "-c", "m.msh"],
             ["info", "nope.msh"], ["info", "-t", "g1.fa"], ["info", "-x", "a.msh"],
             ["paste", "x", "a.msh", "d.msh"], ["info", "-t", "x.msh"], ["info", "-d", "x.msh"], ["paste", "x", "a.msh", "d.msh"],
             ["paste", "y", "a.msh", "b.msh"], ["paste", "z", "a.msh", "p.msh"], ["paste", "w", "a.msh", "s9.msh"],
             ["paste", "-l", "v", "mshlist.txt"], ["info", "-t", "v.msh"], ["paste", "u.msh", "a.msh", "m.msh"], ["info", "-d", "u.msh"],
             ["paste", "t", "a.msh", "missing.msh"], ["paste", "r", "g1.fa"]]
    for args in cases:
        got = {}
        for tag, (exe, d) in dirs.items():
            r = subprocess.run([exe, *args], cwd=d, capture_output=True)
            got[tag] = (r.returncode, r.stdout, r.stderr)
        assert got["ours"] == got["ref"], (args, got["ours"][0], got["ref"][0], got["ours"][2][-200:], got["ref"][2][-200:])


def test_option_refusals_match_the_reference_cli(built, tmp_path):
    """Argument errors are decided before any GPU work, so they can be compared with the reference
    CLI (oracle/_ref/mash-ref) on CPU: same message on stderr, same stdout, same exit status."""
    ref = os.path.join(ROOT, "oracle", "_ref", "mash-ref")
    cli_in = os.path.join(GOLD, "cli", "in")
    if not os.path.exists(ref):
        pytest.skip("reference CLI not built here (make -C oracle refcli)")
    for f in os.listdir(cli_in):
        shutil.copy(os.path.join(cli_in, f), tmp_path)
    subprocess.run([ref, "sketch", "-s", "300", "-o", "a", "g1.fa", "g2.fa", "g3.fa"], cwd=tmp_path, capture_output=True, check=True)
    cases = [["sketch", "-k", "33", "g1.fa"], ["sketch", "-k", "0", "g1.fa"], ["sketch", "-r", "-i", "g1.fa"],
             ["sketch", "-m", "2", "-b", "1G", "reads.fq"], ["sketch", "-q", "g1.fa"], ["sketch", "-k"], ["sketch", "-k", "abc", "g1.fa"],
             ["sketch", "-w", "2", "g1.fa"], ["sketch", "-S", "-1", "g1.fa"], ["sketch", "-z", "AC", "-k", "40", "g1.fa"],
             ["sketch", "-s", "1e3", "-k", "2.5", "g1.fa"], ["dist", "-v", "2", "a.msh", "a.msh"], ["dist", "-d", "2", "a.msh", "a.msh"],
             ["dist", "-k", "16", "a.msh", "g1.fa"], ["triangle", "-v", "3", "a.msh"], ["screen", "-i", "2", "a.msh", "reads.fq"],
             ["screen", "-v", "-1", "a.msh", "reads.fq"]]
    for args in cases:
        got = []
        for exe in (ref, MASH):
            r = subprocess.run([exe, *args], cwd=tmp_path, capture_output=True, stdin=subprocess.DEVNULL, timeout=20)
            got.append((r.returncode, r.stdout, r.stderr))
        assert got[0][0] != 0, args                              # these are refusals
        assert got[0] == got[1], (args, got[0][2][-200:], got[1][2][-200:])


@pytest.mark.gpu
def test_phylip_matrix_from_the_sparse_result(built, tmp_path):
    """`mash triangle` writes its matrix from the pairs that SHARE a hash (mg_compare_tri_sparse_host) and fills the rest of a
    row with the text of {0, min(s, |A| + |B|)} -- distance 1 -- as CommandTriangle.cpp:159-198 would print it; same bytes and
    the same "Max p-value" as the dense path (MASH_AMD_DENSE_MATRIX=1) and as the reference CLI, on tables with empty
    sketches (two of them: distance 0), short ones, copies, and rows that share nothing with anybody; on a collection of one
    species (every pair an exception) the run falls back to the dense path by itself."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import compare_e2e
    ref_cli = compare_e2e.REF if os.path.exists(compare_e2e.REF) else None
    for name, n, s, maker in (("small", 1500, 100, "clusters"), ("large", 4200, 128, "clusters"), ("species", 700, 64, "species")):
        if maker == "clusters":
            table, nhash, lengths = synth.clustered_sketches(n, s, clusters=max(3, n // 60), seed=n, pool=int(1.5 * s), private=int(0.4 * s))
            rnd, rn, _ = synth.random_sketches(40, s, seed=5)
            table[100:140] = rnd
            nhash = nhash.copy()
            nhash[100:140] = rn
            nhash[7] = 0
            nhash[900] = 0
            nhash[33] = s // 3
            table[1200] = table[77]
            nhash[1200] = nhash[77]
        else:
            table, nhash, lengths = synth.species_sketches(n, s, seed=3)
        f = str(tmp_path / f"{name}.msh")
        compare_e2e.write_msh(f, table, nhash, lengths)
        a = run("triangle", f, cwd=tmp_path)
        b = run("triangle", f, cwd=tmp_path, env={"MASH_AMD_DENSE_MATRIX": "1"})
        assert a.stdout == b.stdout and a.stderr == b.stderr, name
        lines = a.stdout.splitlines()
        assert lines[0] == f"\t{n}" and len(lines) == n + 1
        if maker == "clusters":
            assert lines[1 + 900].split("\t")[1 + 7] == "0"            # two empty sketches
            assert lines[1 + 1200].split("\t")[1 + 77] == "0"          # a copy
            assert lines[1 + 139].split("\t")[1:] == ["1"] * 139       # a stranger
        if ref_cli:
            r = subprocess.run([ref_cli, "triangle", f], capture_output=True, text=True, cwd=tmp_path)
            assert r.returncode == 0 and r.stdout == a.stdout and r.stderr == a.stderr, name
