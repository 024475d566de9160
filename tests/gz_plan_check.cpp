// CPU check of csrc/gz_plan.h, the host's part of the device inflate (built and run by tests/test_gz_plan_host.py; needs no GPU).
// zlib plays the device: inflate(..., Z_BLOCK) stops at every block boundary, which gives each member's list of (block start bit,
// text position).  The stand-in "find" gives a chunk with a seek range the first boundary inside it where a dynamic block that is
// not the last begins (what gz_find_kernel looks for), else GZ_NONE; the stand-in "count" walks block ends from a chunk's start to
// the first that is a candidate of its range, to the end of the final block, or past the span limit.  The program drives
// plan -> candidates -> rounds of (count, apply, walk) -> whole members -> layout as gz_inflate_group does and compares the outcome
// with what zlib says about the same bytes: which files are accepted, the text lengths, the members' places, lengths and CRCs.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../phenotypeseeker_amd/csrc/gz_plan.h"

namespace {

int checks = 0, failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            failures++;                                   \
            fprintf(stderr, "FAILED: %s: ", #cond);       \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

typedef std::vector<uint8_t> Bytes;

// FASTQ-like text: compressible, but with enough entropy for many dynamic blocks
Bytes make_text(size_t n, uint32_t seed)
{
    Bytes t;
    uint32_t s = seed * 2654435761u + 1;
    auto rnd = [&] { return (s = s * 1664525u + 1013904223u) >> 16; };
    for (int r = 0; t.size() < n; r++) {
        char head[32];
        const int hl = snprintf(head, sizeof head, "@read%d/%u\n", r, rnd() % 97);
        t.insert(t.end(), head, head + hl);
        for (int i = 0; i < 100; i++) t.push_back("ACGT"[rnd() & 3]);
        t.push_back('\n'); t.push_back('+'); t.push_back('\n');
        for (int i = 0; i < 100; i++) t.push_back((uint8_t)('!' + rnd() % 41));
        t.push_back('\n');
    }
    t.resize(n);
    return t;
}

// one gzip member; bgzf: with the BC extra field, BSIZE filled in; flush_every: a Z_FULL_FLUSH after every so many bytes of text
Bytes gz_member(const Bytes &text, int level, int mem_level, size_t flush_every, bool bgzf)
{
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, level, Z_DEFLATED, 15 + 16, mem_level, Z_DEFAULT_STRATEGY) != Z_OK) abort();
    gz_header gh;
    uint8_t extra[6] = {'B', 'C', 2, 0, 0, 0};
    if (bgzf) {
        memset(&gh, 0, sizeof gh);
        gh.extra = extra;
        gh.extra_len = 6;
        gh.os = 255;
        deflateSetHeader(&z, &gh);
    }
    Bytes out(deflateBound(&z, (uLong)text.size()) + 64 + (flush_every ? text.size() / flush_every * 16 : 0));
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    size_t at = 0;
    int rc = Z_OK;
    while (rc != Z_STREAM_END) {
        const size_t step = flush_every ? std::min(flush_every, text.size() - at) : text.size() - at;
        z.next_in = const_cast<Bytef *>(text.data() + at);
        z.avail_in = (uInt)step;
        at += step;
        rc = deflate(&z, at == text.size() ? Z_FINISH : Z_FULL_FLUSH);
        if (rc != Z_OK && rc != Z_STREAM_END) abort();
    }
    out.resize(z.total_out);
    deflateEnd(&z);
    if (bgzf) {
        out[16] = (uint8_t)((out.size() - 1) & 0xff);
        out[17] = (uint8_t)((out.size() - 1) >> 8);
    }
    return out;
}

// ---- what zlib says about a file -------------------------------------------------------------------------------------
struct Member {
    size_t deflate_at = 0;
    std::vector<uint64_t> bound, pos;   // bit (in the file) and text position of every block boundary: start, block ends
    Bytes text;
    uint64_t end_bit() const { return bound.back(); }
};
struct Case {
    std::string name;
    Bytes bytes;
    std::vector<Member> members;
    bool accept = true;
    size_t text_len() const { size_t n = 0; for (const Member &m : members) n += m.text.size(); return n; }
};

uint32_t bits_at(const Bytes &d, uint64_t bit, int n)
{
    uint32_t v = 0;
    for (int i = 0; i < n; i++, bit++) v |= (uint32_t)((d[bit >> 3] >> (bit & 7)) & 1) << i;
    return v;
}

// appends the member to the case and records its block boundaries
void add_member(Case &c, const Bytes &text, const Bytes &gz)
{
    const size_t at = c.bytes.size();
    c.bytes.insert(c.bytes.end(), gz.begin(), gz.end());
    Member m;
    GzMemberHead h;
    if (!gz_parse_member_header(c.bytes.data(), c.bytes.size(), at, &h)) abort();
    m.deflate_at = h.deflate_at;
    m.text = text;
    Bytes out(text.size() + 64);
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) abort();
    z.next_in = c.bytes.data() + m.deflate_at;
    z.avail_in = (uInt)(c.bytes.size() - m.deflate_at);
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    m.bound.push_back(m.deflate_at * 8);
    m.pos.push_back(0);
    for (;;) {
        const int rc = inflate(&z, Z_BLOCK);
        if (rc == Z_STREAM_END) break;
        if (rc != Z_OK) abort();
        if (z.data_type & 128) {
            m.bound.push_back((m.deflate_at + z.total_in) * 8 - (uint64_t)(z.data_type & 63));
            m.pos.push_back(z.total_out);
        }
    }
    if (z.total_out != text.size() || (!text.empty() && memcmp(out.data(), text.data(), text.size()) != 0)) abort();
    if ((m.end_bit() + 7) / 8 != m.deflate_at + z.total_in) abort();
    inflateEnd(&z);
    c.members.push_back(m);
}

// a boundary of a member (not its end): does a dynamic block that is not the last begin there?
bool is_candidate(const Case &c, const Member &m, size_t k) { return k + 1 < m.bound.size() && bits_at(c.bytes, m.bound[k], 3) == 4; }
bool is_final(const Case &c, const Member &m, size_t k) { return bits_at(c.bytes, m.bound[k], 1) == 1; }

// ---- the device's part -------------------------------------------------------------------------------------------------
uint64_t standin_find(const Case &c, uint64_t image_bit, uint64_t from, uint64_t to)
{
    uint64_t best = GZ_NONE;
    for (const Member &m : c.members)
        for (size_t k = 0; k + 1 < m.bound.size(); k++) {
            const uint64_t b = image_bit + m.bound[k];
            if (b >= from && b < to && b < best && is_candidate(c, m, k)) best = b;
        }
    return best;
}

struct Counted {
    uint64_t out_len = 0, n_rec = 0, end_bit = 0;
    int32_t link = GZ_ERROR;
};
// (the order of the tests at a block boundary is gz_decode_kernel<false>'s: final, candidate, span)
Counted standin_count(const Case &c, uint64_t image_bit, uint64_t start, const GzCands &cands, std::pair<uint32_t, uint32_t> range, uint64_t max_span_bits)
{
    Counted r;
    r.end_bit = start;
    for (const Member &m : c.members)
        for (size_t k0 = 0; k0 + 1 < m.bound.size(); k0++) {
            if (image_bit + m.bound[k0] != start) continue;
            uint32_t nc = range.first;
            for (size_t k = k0;; k++) {
                const uint64_t bit = image_bit + m.bound[k];
                r.end_bit = bit;
                r.out_len = m.pos[k] - m.pos[k0];
                if (k + 1 == m.bound.size()) {
                    r.link = GZ_FINAL;
                    break;
                }
                while (nc < range.second && cands.bit[nc] < bit) nc++;
                if (nc < range.second && cands.bit[nc] == bit) {
                    r.link = (int32_t)nc;
                    break;
                }
                if (bit - start > max_span_bits) {
                    r.link = GZ_OVERRUN;
                    break;
                }
                if (is_final(c, m, k) != (k + 2 == m.bound.size())) abort();   // (the model itself: the last block is the final one)
            }
            r.n_rec = r.out_len / 7;
            return r;
        }
    return r;   // no block begins at `start`: a real decoder meets an error or runs into the span limit
}

struct Outcome {
    GzPlan plan;
    GzTextLayout L;
    int rounds = 0;
    size_t regular_chunks = 0;
    int planted_chunk = -1;
};

// plant: the n-th chunk with a seek range "finds" a start three bits into its range, where no block begins
Outcome run_group(const std::vector<const Case *> &g, size_t chunk_knob, int max_rounds, size_t max_span, int plant = -1)
{
    std::vector<const uint8_t *> data;
    std::vector<size_t> sizes;
    size_t bytes = 0;
    for (const Case *c : g) {
        data.push_back(c->bytes.data());
        sizes.push_back(c->bytes.size());
        bytes += c->bytes.size();
    }
    const size_t chunk = gz_chunk_bytes(bytes, 65536, chunk_knob);
    Outcome o;
    o.plan = gz_plan_chunks((int)g.size(), data.data(), sizes.data(), chunk);
    GzPlan &p = o.plan;
    o.regular_chunks = p.ch.size();
    int seeking = 0;
    for (size_t c = 0; c < p.ch.size(); c++) {
        GzChunk &k = p.ch[c];
        if (k.seek_to <= k.seek_from) continue;
        k.start_bit = standin_find(*g[(size_t)k.file], p.files[(size_t)k.file].at * 8, k.seek_from, k.seek_to);
        if (seeking++ == plant) {
            k.start_bit = k.seek_from + 3;
            o.planted_chunk = (int)c;
        }
    }
    const uint64_t max_span_bits = (uint64_t)std::max<size_t>(chunk * 8, max_span) * 8;
    GzCands cands;
    while (!p.todo.empty()) {
        if (++o.rounds > max_rounds) {
            gz_decline_unfinished(p);
            break;
        }
        cands.rebuild(p);
        const size_t m = p.todo.size();
        std::vector<uint64_t> r_len(m, 0), r_nrec(m, 0), r_ebit(m, 0);
        std::vector<int32_t> r_link(m, (int32_t)0xfefefefe);
        for (size_t j = 0; j < m; j++) {
            const GzChunk &k = p.ch[(size_t)p.todo[j]];
            const GzFile &f = p.files[(size_t)k.file];
            if (!f.device_ok || k.start_bit == GZ_NONE) continue;
            const Counted r = standin_count(*g[(size_t)k.file], f.at * 8, k.start_bit, cands, cands.range(k), max_span_bits);
            r_len[j] = r.out_len; r_nrec[j] = r.n_rec; r_ebit[j] = r.end_bit; r_link[j] = r.link;
        }
        gz_apply_round(p, cands, r_len.data(), r_nrec.data(), r_ebit.data(), r_link.data());
        gz_walk_chains(p);
    }
    gz_keep_whole_members(p);
    o.L = gz_layout_text(p);
    return o;
}

// every assertion of the issue's list, for every file of the group
void verify(const std::vector<const Case *> &g, const Outcome &o, const char *what)
{
    const GzPlan &p = o.plan;
    const GzTextLayout &L = o.L;
    CHECK(L.members_whole(), "%s", what);
    CHECK(L.total % 64 == 0 && L.file_first.size() >= 1 && L.file_first.back() == L.order.size(), "%s", what);
    CHECK(L.c_off.size() == L.order.size() && L.c_rec.size() == L.order.size() && L.members_only.size() + 1 == L.file_first.size(), "%s", what);
    size_t q = 0;   // the next member of the layout
    uint64_t prev_end = GZ_WIN, rec = 0;
    int slot = 0;
    for (size_t i = 0; i < g.size(); i++) {
        const Case &c = *g[i];
        const GzFile &f = p.files[i];
        const uint64_t image_bit = f.at * 8;
        CHECK(f.device_ok == c.accept, "%s / %s: device_ok %d", what, c.name.c_str(), (int)f.device_ok);
        if (!f.device_ok) continue;
        CHECK(f.nul_slot == slot && L.file_first[(size_t)slot] <= L.file_first[(size_t)slot + 1], "%s / %s", what, c.name.c_str());
        CHECK(f.out_off % 64 == 0 && f.out_off >= prev_end, "%s / %s: out_off %llu", what, c.name.c_str(), (unsigned long long)f.out_off);
        uint64_t sum = 0;
        bool all_true = true;
        size_t j = L.file_first[(size_t)slot];
        CHECK(L.file_first[(size_t)slot + 1] - j == f.chain.size(), "%s / %s", what, c.name.c_str());
        for (size_t k = 0; k < f.chain.size(); k++, j++) {
            const GzChunk &ck = p.ch[(size_t)f.chain[k]];
            CHECK(L.order[j] == f.chain[k] && L.c_off[j] == f.out_off + sum && L.c_rec[j] == rec, "%s / %s: chunk %zu of the chain", what, c.name.c_str(), k);
            CHECK(f.chain[k] != o.planted_chunk, "%s / %s: the planted start is in the chain", what, c.name.c_str());
            bool member_start = false, boundary = false;
            for (const Member &m : c.members) {
                member_start = member_start || ck.start_bit == image_bit + m.bound[0];
                for (size_t b = 0; b + 1 < m.bound.size(); b++) boundary = boundary || ck.start_bit == image_bit + m.bound[b];
            }
            CHECK(boundary && ck.true_start == member_start, "%s / %s: chunk %zu of the chain: true_start %d", what, c.name.c_str(), k, (int)ck.true_start);
            if (k + 1 < f.chain.size() && ck.link >= 0) CHECK(p.ch[(size_t)f.chain[k + 1]].start_bit == ck.end_bit, "%s / %s: chunk %zu", what, c.name.c_str(), k);
            all_true = all_true && member_start;
            sum += ck.out_len;
            rec += ck.n_rec;
        }
        CHECK(sum == c.text_len() && f.out_len == sum, "%s / %s: %llu bytes of text, zlib %zu", what, c.name.c_str(), (unsigned long long)sum, c.text_len());
        CHECK((L.members_only[(size_t)slot] != 0) == all_true, "%s / %s: members_only", what, c.name.c_str());
        uint64_t begin = f.out_off;
        for (const Member &m : c.members) {
            const bool have = q < L.m_begin.size() && q < L.m_len.size() && q < L.m_crc.size();
            CHECK(have && L.m_file[q] == (int)i && L.m_begin[q] == begin && L.m_len[q] == m.text.size(), "%s / %s: member at %llu", what, c.name.c_str(),
                  (unsigned long long)begin);
            CHECK(have && L.m_crc[q] == (uint32_t)crc32(crc32(0, nullptr, 0), m.text.data(), (uInt)m.text.size()), "%s / %s: member crc", what, c.name.c_str());
            begin += m.text.size();
            q++;
        }
        prev_end = f.out_off + f.out_len;
        slot++;
    }
    CHECK(q == L.m_begin.size() && rec == L.total_rec && L.total >= prev_end && (size_t)slot + 1 == L.file_first.size(), "%s", what);
}

Case single(const char *name, const Bytes &text, int level, int mem_level, size_t flush_every)
{
    Case c;
    c.name = name;
    add_member(c, text, gz_member(text, level, mem_level, flush_every, false));
    return c;
}

// `n` members of `each` bytes of text, `between` / `after` zero bytes of padding
Case members(const char *name, int n, size_t each, size_t between, size_t after, int mem_level = 8)
{
    Case c;
    c.name = name;
    for (int i = 0; i < n; i++) {
        const Bytes text = make_text(each + 101 * (size_t)i, 40 + (uint32_t)i);
        add_member(c, text, gz_member(text, 6, mem_level, 0, false));
        if (i + 1 < n) c.bytes.insert(c.bytes.end(), between, 0);
    }
    c.bytes.insert(c.bytes.end(), after, 0);
    return c;
}

Case bgzf(const char *name, size_t total, size_t block)
{
    Case c;
    c.name = name;
    const Bytes text = make_text(total, 77);
    for (size_t at = 0; at < total; at += block) {
        const Bytes part(text.begin() + (long)at, text.begin() + (long)std::min(at + block, total));
        add_member(c, part, gz_member(part, 6, 8, 0, true));
    }
    add_member(c, Bytes(), gz_member(Bytes(), 6, 8, 0, true));   // the end-of-file member
    return c;
}

}  // namespace

int main()
{
    const size_t max_span = 1 << 16;
    std::vector<Case> cases;
    cases.push_back(single("one member, full flushes", make_text(300000, 1), 6, 8, 8000));
    cases.push_back(single("one member", make_text(300000, 2), 6, 8, 0));
    cases.push_back(single("one member, small blocks", make_text(120000, 3), 6, 3, 0));
    cases.push_back(single("empty text", Bytes(), 6, 8, 0));
    cases.push_back(members("two members", 2, 60000, 0, 0));
    cases.push_back(members("two members, padded", 2, 60000, 11, 37));
    cases.push_back(members("five members", 5, 30000, 0, 0, 4));
    cases.push_back(members("five members, padded", 5, 30000, 5, 64, 4));
    cases.push_back(bgzf("bgzf", 100000, 6000));
    {
        Case c = bgzf("bgzf, one BSIZE off by one", 100000, 6000);
        GzMemberHead h;
        gz_parse_member_header(c.bytes.data(), c.bytes.size(), 0, &h);
        c.bytes[h.bsize + 16]++;   // (the second member's)
        c.accept = false;
        cases.push_back(c);
    }
    {
        Case c = single("truncated inside the trailer", make_text(50000, 5), 6, 8, 0);
        c.bytes.resize(c.bytes.size() - 5);
        c.accept = false;
        cases.push_back(c);
    }
    {
        Case c = single("wrong ISIZE", make_text(50000, 6), 6, 8, 0);
        c.bytes[c.bytes.size() - 4] ^= 1;
        c.accept = false;
        cases.push_back(c);
    }
    {
        Case c = single("stored blocks only", make_text(300000, 7), 0, 8, 0);
        c.accept = false;   // no dynamic header to find: the chain runs into the span limit
        cases.push_back(c);
    }
    const size_t chunks[2] = {4096, 20000};
    // every case on its own, then all of them as one group (images at offsets, declined files between accepted ones)
    std::vector<const Case *> all;
    for (const Case &c : cases) all.push_back(&c);
    for (size_t chunk : chunks) {
        for (const Case &c : cases) {
            const std::string what = c.name + " alone, chunk " + std::to_string(chunk);
            verify({&c}, run_group({&c}, chunk, 24, max_span), what.c_str());
        }
        const std::string what = "all in one group, chunk " + std::to_string(chunk);
        const Outcome o = run_group(all, chunk, 24, max_span);
        verify(all, o, what.c_str());
        CHECK(o.rounds >= 2, "%s: %d rounds", what.c_str(), o.rounds);   // (members in the middle of files: more than one round)
    }
    // the stored-only file is declined because of the span limit, not otherwise: with room enough it is accepted
    {
        Case c = cases.back();
        c.accept = true;
        verify({&c}, run_group({&c}, 4096, 24, (size_t)1 << 20), "stored blocks only, span limit 1 MiB");
    }
    // a planted false-positive start: never in a chain, the text unaffected
    for (int plant : {0, 2, 5}) {
        const Case &c = cases[0];
        const Outcome o = run_group({&c}, 4096, 24, max_span, plant);
        CHECK(o.planted_chunk >= 0 && o.plan.ch[(size_t)o.planted_chunk].counted && o.plan.ch[(size_t)o.planted_chunk].link == GZ_ERROR, "plant %d", plant);
        verify({&c}, o, "planted start");
    }
    // a second member whose data start is exactly a found chunk start: the chunk is adopted, no extra chunk, one round ...
    {
        const Case c = members("two members, second starts a chunk", 2, 60000, 0, 0);
        GzMemberHead h;
        gz_parse_member_header(c.bytes.data(), c.bytes.size(), 0, &h);
        const size_t chunk = (c.members[1].deflate_at - h.deflate_at) & ~(size_t)3;   // the second cut falls into the second member's header
        const Outcome o = run_group({&c}, chunk, 24, max_span);
        verify({&c}, o, "second member adopted");
        const GzFile &f = o.plan.files[0];
        CHECK(o.plan.ch.size() == o.regular_chunks && o.rounds == 1, "adopted: %zu chunks (%zu regular), %d rounds", o.plan.ch.size(), o.regular_chunks, o.rounds);
        CHECK(f.chain.size() >= 2 && o.plan.ch[1].start_bit == c.members[1].bound[0] && o.plan.ch[1].true_start, "adopted: chunk 1 starts the second member");
        bool in_chain = false;
        for (int k : f.chain) in_chain = in_chain || k == 1;
        CHECK(in_chain, "adopted: chunk 1 is in the chain");
        // ... and where it is not (the cut falls just behind it, its start lies in the range of no search): one extra chunk, one more round
        const Outcome o2 = run_group({&c}, chunk + 4, 24, max_span);
        verify({&c}, o2, "second member by an extra chunk");
        CHECK(o2.plan.ch.size() == o2.regular_chunks + 1 && o2.rounds == 2, "extra: %zu chunks (%zu regular), %d rounds", o2.plan.ch.size(), o2.regular_chunks, o2.rounds);
    }
    // three members: three rounds; one round allowed: declined
    {
        Case c = members("three small members", 3, 3000, 0, 0);
        const Outcome o = run_group({&c}, 4096, 24, max_span);
        verify({&c}, o, "three members");
        CHECK(o.rounds == 3, "three members: %d rounds", o.rounds);
        c.accept = false;
        verify({&c}, run_group({&c}, 4096, 1, max_span), "three members, one round");
    }
    // the whole-members rule on chains no valid stream gives: per chunk {true_start, link}
    {
        struct K { bool true_start; int32_t link; };
        const struct { std::vector<K> chain; bool whole; } chains[] = {
            {{{true, GZ_FINAL}}, true},
            {{{true, 1}, {false, GZ_FINAL}, {true, GZ_FINAL}}, true},
            {{}, false},                                      // no chunk at all
            {{{false, GZ_FINAL}}, false},                     // does not begin with a member's start
            {{{true, 1}, {false, 2}}, false},                 // ends inside a member
            {{{true, 1}, {true, GZ_FINAL}}, false},           // a member's start inside a member
            {{{true, GZ_FINAL}, {false, GZ_FINAL}}, false},   // a second member that does not begin with one
        };
        for (const auto &c : chains) {
            GzPlan p;
            p.files.resize(1);
            for (const K &k : c.chain) {
                GzChunk ch;
                ch.file = 0; ch.start_bit = 0; ch.seek_from = ch.seek_to = 0; ch.true_start = k.true_start; ch.link = k.link; ch.counted = true;
                p.files[0].chain.push_back((int)p.ch.size());
                p.ch.push_back(ch);
            }
            gz_keep_whole_members(p);
            CHECK(p.files[0].device_ok == c.whole, "whole-members rule, chain of %zu", c.chain.size());
        }
    }
    // the chunk size: the knob, else bytes over lanes within 16 KB .. 4 MB, a multiple of 4
    CHECK(gz_chunk_bytes(1 << 20, 65536, 0) == (16 << 10) && gz_chunk_bytes((size_t)1 << 40, 65536, 0) == (4 << 20), "chunk bounds");
    CHECK(gz_chunk_bytes((size_t)65536 * 100001, 65536, 0) == 100004 && gz_chunk_bytes(1 << 20, 65536, 4097) == 4100, "chunk rounding");
    printf("gz_plan_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
