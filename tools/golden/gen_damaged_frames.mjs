// tools/golden/gen_damaged_frames.mjs — records what the reference's decompressBuffer does with
// damaged frames, by EXECUTING the reference JavaScript in the build container. Run:
//   node tools/golden/gen_damaged_frames.mjs /root/reference tests/golden
// It writes tests/golden/damaged_frames.json and nothing else (manifest.json is gen_golden.mjs's).
//
// This script contains only our own input generators, edit lists and harness code. It imports the
// reference modules by absolute path at run time; nothing of the reference is copied. The fixture
// holds recipes and outcomes, no frame bytes: a base frame is named by its content (generator,
// seed, length per part) and encoder flags and rebuilt in the tests by oracle.compress_frame (the
// golden tests pin its bytes; frame_len / frame_xxh here check it again), and a case is the list
// of pieces its damaged frame is put together from: [a, b] = base[a:b], a string = hex bytes
// (written out in a shorter form, see the end of this file; tests/damaged_common.py reads it).
//
// Every case is decoded with verifyChecksum true and false, each twice: once after the reference's
// module-level 4 MiB workspace was filled with 0x00 and once after 0xFF (by decoding an unsized frame
// of 4 MiB of that byte). A case whose outcomes differ between the fills returns bytes of earlier calls
// (an unsized frame cut inside a block's last literal run): recorded as unspecified, no outcome. So is a
// case whose error is a failed allocation, except the 2^48 content size.
import fs from 'fs';
import path from 'path';

const REF = process.argv[2] || '/root/reference';
const OUT = process.argv[3] || 'tests/golden';
const BLOCK = 65536;
const UNSPEC_CAP = 0.15;      // of an unsized base frame's cases; sized frames: none (see main)

async function main() {
const { xxHash32 } = await import(path.join(REF, 'src/xxhash32/xxhash32.js'));
const { compressBuffer } = await import(path.join(REF, 'src/buffer/bufferCompress.js'));
const { decompressBuffer } = await import(path.join(REF, 'src/buffer/bufferDecompress.js'));

// ---- seeded generators (the definitions of gen_golden.mjs / oracle orc_generate) ----
function rng(seed) { let x = (seed >>> 0) || 1; return () => { x ^= x << 13; x >>>= 0; x ^= x >>> 17; x ^= x << 5; x >>>= 0; return x; }; }
function gen(kind, seed, n) {
    const r = rng(seed), b = new Uint8Array(n); let i = 0;
    switch (kind) {
        case 'random': for (i = 0; i < n; i += 4) { const v = r(); for (let k = 0; k < 4 && i + k < n; k++) b[i + k] = (v >>> (8 * k)) & 255; } break;
        case 'tiles216': {
            const t = new Uint8Array(216 * 64); for (let k = 0; k < t.length; k++) t[k] = r() & 255;
            while (i < n) { const base = 64 * (r() % 216); for (let k = 0; k < 64 && i < n; k++) b[i++] = t[base + k]; }
            break;
        }
        case 'text': {
            const words = 'the of and to in is was for on that with as by at from his an were are which this be or has had not but it its'.split(' ');
            while (i < n) {
                const v = r(); const w = words[v % words.length];
                for (let k = 0; k < w.length && i < n; k++) b[i++] = w.charCodeAt(k);
                if (i < n) b[i++] = ((v >>> 16) % 11 === 0) ? 10 : 32;
            }
            break;
        }
        default: throw new Error('bad kind ' + kind);
    }
    return b;
}
// spec XXH32 (the block checksum of the LZ4 frame format; the reference's own hash is a variant)
function xxh32std(b) {
    const P1 = 2654435761, P2 = 2246822519, P3 = 3266489917, P4 = 668265263, P5 = 374761393;
    const rot = (x, r) => (x << r) | (x >>> (32 - r));
    const rd = (p) => (b[p] | (b[p + 1] << 8) | (b[p + 2] << 16) | (b[p + 3] << 24));
    const n = b.length; let p = 0, h;
    if (n >= 16) {
        let v1 = (P1 + P2) | 0, v2 = P2 | 0, v3 = 0, v4 = -P1 | 0;
        for (; p + 16 <= n; p += 16) {
            v1 = Math.imul(rot((v1 + Math.imul(rd(p), P2)) | 0, 13), P1);
            v2 = Math.imul(rot((v2 + Math.imul(rd(p + 4), P2)) | 0, 13), P1);
            v3 = Math.imul(rot((v3 + Math.imul(rd(p + 8), P2)) | 0, 13), P1);
            v4 = Math.imul(rot((v4 + Math.imul(rd(p + 12), P2)) | 0, 13), P1);
        }
        h = (rot(v1, 1) + rot(v2, 7) + rot(v3, 12) + rot(v4, 18)) | 0;
    } else h = P5 | 0;
    h = (h + n) | 0;
    for (; p + 4 <= n; p += 4) h = Math.imul(rot((h + Math.imul(rd(p), P3)) | 0, 17), P4);
    for (; p < n; p++) h = Math.imul(rot((h + Math.imul(b[p], P5)) | 0, 11), P1);
    h ^= h >>> 15; h = Math.imul(h, P2); h ^= h >>> 13; h = Math.imul(h, P3); h ^= h >>> 16;
    return h >>> 0;
}
const hex = (u) => (u >>> 0).toString(16).padStart(8, '0');
const le32 = (v) => Buffer.from([v & 255, (v >>> 8) & 255, (v >>> 16) & 255, (v >>> 24) & 255]).toString('hex');
const rd32 = (f, p) => (f[p] | (f[p + 1] << 8) | (f[p + 2] << 16) | (f[p + 3] << 24)) >>> 0;
function concat(parts) {
    const n = parts.reduce((a, b) => a + b.length, 0), g = new Uint8Array(n);
    let o = 0; for (const x of parts) { g.set(x, o); o += x.length; }
    return g;
}

// ---- base frames ----------------------------------------------------------------------------
const CONTENTS = {
    A: [['text', 101, 65536], ['random', 102, 65536], ['tiles216', 103, 40000]],   // compressed, stored, compressed tail
    B: [['text', 111, 70000], ['random', 112, 65536], ['tiles216', 113, 40000]],   // the middle block: compressed, a ~60 KB literal run
    E: [],
};
const VARIANTS = [   // name, independent, content size, content checksum, block checksums
    ['is', true, true, false, false], ['iu', true, false, false, false], ['ds', false, true, false, false],
    ['du', false, false, false, false], ['isc', true, true, true, false], ['isb', true, true, false, true]];

// the records of an undamaged frame: header length, [{w: size word position, p: payload, n, stored, e: record end}], EndMark
function layout(f) {
    const flg = f[4];
    let pos = 6 + ((flg & 8) ? 8 : 0) + ((flg & 1) ? 4 : 0) + 1;
    const L = { hdr: pos, recs: [], flg, bcs: (flg & 0x10) ? 4 : 0 };
    for (;;) {
        const v = rd32(f, pos);
        if (v === 0) break;
        const n = v & 0x7FFFFFFF;
        L.recs.push({ w: pos, p: pos + 4, n, stored: (v & 0x80000000) !== 0, e: pos + 4 + n + L.bcs });
        pos += 4 + n + L.bcs;
    }
    L.end = pos; L.sum = pos + 4; L.len = f.length;
    return L;
}
function withBlockChecksums(f) {   // re-laid like oracle orc_compress_frame_ex(block_checksum=1): FLG 0x10, HC again
    const L = layout(f);
    const hdr = Uint8Array.from(f.subarray(0, L.hdr));
    hdr[4] |= 0x10;
    hdr[L.hdr - 1] = (xxHash32(hdr.subarray(4, L.hdr - 1), 0) >>> 8) & 0xFF;
    const parts = [hdr];
    for (const r of L.recs) {
        parts.push(f.subarray(r.w, r.e));
        parts.push(Uint8Array.from(Buffer.from(le32(xxh32std(f.subarray(r.p, r.p + r.n))), 'hex')));
    }
    parts.push(f.subarray(L.end));
    return concat(parts);
}

// ---- the edit list of one base frame ----------------------------------------------------------
function edits(f, L, seed) {
    const r = rng(seed), N = f.length, cases = [];
    const add = (k, p) => cases.push({ k, p });
    const setAt = (k, pos, bytesHex) => add(k, [[0, pos], bytesHex, [pos + bytesHex.length / 2, N]]);
    const cuts = new Set();
    const cut = (k, n) => { if (n >= 0 && n <= N && !cuts.has(n)) { cuts.add(n); add(k, [[0, n]]); } };
    // truncation: 0..32, +-8 around every record boundary, the EndMark and the checksum, ~40 seeded per block
    for (let n = 0; n <= 32; n++) cut('cut_head', n);
    const marks = L.recs.map((x) => x.w).concat([L.end, L.sum, N]);
    for (const m of marks) for (let d = -8; d <= 8; d++) cut('cut_edge', m + d);
    for (const x of L.recs) for (let k = 0; k < 40; k++) cut(x.stored ? 'cut_stored' : 'cut_block', x.p + r() % x.n);
    // header: FLG bits, BD ids and reserved bits, the header checksum byte, the content size
    for (let b = 0; b < 8; b++) setAt('hdr_flg', 4, Buffer.from([f[4] ^ (1 << b)]).toString('hex'));
    for (let id = 0; id < 8; id++) setAt('hdr_bd', 5, Buffer.from([(f[5] & 0x8F) | (id << 4)]).toString('hex'));
    for (const m of [0x80, 0x08, 0x04, 0x02, 0x01]) setAt('hdr_bd', 5, Buffer.from([f[5] ^ m]).toString('hex'));
    for (const m of [0x01, 0xFF]) setAt('hdr_hc', L.hdr - 1, Buffer.from([f[L.hdr - 1] ^ m]).toString('hex'));
    if (L.flg & 8) {
        const size = rd32(f, 6);
        for (const v of [0, size - 1, size + 1, size - BLOCK, size + BLOCK]) setAt('hdr_size', 6, le32(v) + '00000000');
        setAt('hdr_size_2p48', 6, '000000000000' + '0100');
    }
    // size words: stored bit, +-1, +-4, +-65536, 0, 0x7FFFFFFF, 0xFFFFFFFF
    for (const x of L.recs) {
        const w = rd32(f, x.w);
        const vals = [(w ^ 0x80000000) >>> 0, w + 1, w - 1, w + 4, w - 4, w + 65536, w - 65536, 0, 0x7FFFFFFF, 0xFFFFFFFF];
        for (const v of vals) setAt('word', x.w, le32(v >>> 0));
    }
    // structure
    add('no_endmark', [[0, L.end], [L.sum, N]]);
    add('no_endmark', [[0, L.end]]);
    for (let g = 1; g <= 8; g++) { let h = ''; for (let k = 0; k < g; k++) h += Buffer.from([r() & 255]).toString('hex'); add('garbage', [[0, N], h]); }
    const rec = L.recs;
    for (let k = 0; k < rec.length; k++) {
        add('dup', [[0, rec[k].e], [rec[k].w, N]]);
        add('drop', [[0, rec[k].w], [rec[k].e, N]]);
    }
    for (let a = 0; a < rec.length; a++) for (let b = a + 1; b < rec.length; b++)
        add('swap', [[0, rec[a].w], [rec[b].w, rec[b].e], [rec[a].e, rec[b].w], [rec[a].w, rec[a].e], [rec[b].e, N]]);
    // a stored block of 1000 frame bytes past the content (before the EndMark), and one in front
    const stored = le32((1000 | 0x80000000) >>> 0);
    const tail = L.bcs ? 'a55ac301' : '';
    if (rec.length) {
        add('stored_past', [[0, L.end], stored, [L.hdr, L.hdr + 1000], tail, [L.end, N]]);
        add('stored_front', [[0, L.hdr], stored, [L.hdr, L.hdr + 1000], tail, [L.hdr, N]]);
    }
    // payload: ~30 seeded single-byte edits per compressed block
    for (const x of L.recs) if (!x.stored) for (let k = 0; k < 30; k++) {
        const pos = x.p + r() % x.n;
        setAt('payload', pos, Buffer.from([f[pos] ^ (1 + r() % 255)]).toString('hex'));
    }
    // checksums
    if (L.flg & 4) for (let k = 0; k < 4; k++) for (const m of [0x01, 0x80]) setAt('csum', L.sum + k, Buffer.from([f[L.sum + k] ^ m]).toString('hex'));
    if (L.bcs) for (const x of L.recs) for (const k of [0, 3]) setAt('bsum', x.e - 4 + k, Buffer.from([f[x.e - 4 + k] ^ 0x40]).toString('hex'));
    add('whole', [[0, N]]);
    return cases;
}

function build(f, pieces) {
    return concat(pieces.map((p) => typeof p === 'string' ? Uint8Array.from(Buffer.from(p, 'hex')) : f.subarray(p[0], p[1])));
}

// ---- the two workspace fills ----------------------------------------------------------------
const fills = [0x00, 0xFF].map((v) => compressBuffer(new Uint8Array(4194304).fill(v), null, 4194304, true, false, false));
function outcome(g, verify, fill) {
    decompressBuffer(fills[fill]);
    try {
        const out = decompressBuffer(g, null, verify);
        return [1, out.length, hex(xxHash32(out, 0))];
    } catch (e) {
        return [0, e.name, String(e.message)];
    }
}
const isAlloc = (o) => o[0] === 0 && o[1] === 'RangeError' && /Invalid typed array length|allocation failed/.test(o[2]);

const doc = { generator: 'tools/golden/gen_damaged_frames.mjs', node: process.version, block: BLOCK, contents: CONTENTS, bases: [] };
let seed = 9000;
for (const cname of ['A', 'B', 'E']) {
    const input = concat(CONTENTS[cname].map(([k, s, n]) => gen(k, s, n)));
    for (const [vname, indep, size, csum, bsum] of (cname === 'E' ? [VARIANTS[1]] : VARIANTS)) {
        let f = compressBuffer(input, null, BLOCK, indep, csum, size);
        if (bsum) f = withBlockChecksums(f);
        const L = layout(f);
        let cases = edits(f, L, ++seed);
        let unspec = 0;
        for (const c of cases) {
            const g = build(f, c.p);
            const o = [[outcome(g, true, 0), outcome(g, true, 1)], [outcome(g, false, 0), outcome(g, false, 1)]];
            const same = JSON.stringify(o[0][0]) === JSON.stringify(o[0][1]) && JSON.stringify(o[1][0]) === JSON.stringify(o[1][1]);
            if (!same || ((isAlloc(o[0][0]) || isAlloc(o[1][0])) && c.k !== 'hdr_size_2p48')) {
                c.u = 1; unspec++;
                // a frame decoded into its own zero-filled result cannot depend on earlier calls
                if (!same && (g[4] & 8) && g.length >= 14 && (rd32(g, 6) || rd32(g, 10))) throw new Error('sized frame, unspecified: ' + JSON.stringify(c));
            } else { c.v = o[0][0]; c.n = o[1][0]; }
        }
        // over the cap: thin the truncations inside blocks (never raise the cap)
        for (let k = cases.length - 1; k >= 0 && unspec > UNSPEC_CAP * cases.length; k--)
            if (cases[k].u && cases[k].k === 'cut_block') { cases.splice(k, 1); unspec--; }
        doc.bases.push({ name: cname + '_' + vname, content: cname, indep, size, csum, bsum, frame_len: f.length, frame_xxh: hex(xxHash32(f, 0)),
            unspecified: unspec, cases });
        console.log(cname + '_' + vname, 'frame', f.length, 'cases', cases.length, 'unspecified', unspec);
    }
}
// compact: one line per base frame. A case is [kind, recipe, outcome verified, outcome unverified]: kind and
// outcomes index the base's "kinds" and "outcomes" lists (-1, -1: unspecified); the recipe is a length L (the
// frame cut to L bytes), [pos, hex] (those bytes written over base[pos..]) or the list of pieces.
function recipe(p, N) {
    if (p.length === 1 && p[0][0] === 0) return p[0][1];
    if (p.length === 3 && typeof p[1] === 'string' && p[0][0] === 0 && p[2][1] === N && p[2][0] === p[0][1] + p[1].length / 2) return [p[0][1], p[1]];
    return p;
}
let s = '{"generator":' + JSON.stringify(doc.generator) + ',"node":' + JSON.stringify(doc.node) + ',"block":' + BLOCK +
    ',"contents":' + JSON.stringify(doc.contents) + ',"bases":[\n';
s += doc.bases.map((b) => {
    const { cases, ...head } = b;
    const kinds = [], outcomes = [], seen = new Map();
    const oidx = (o) => { const key = JSON.stringify(o); if (!seen.has(key)) { seen.set(key, outcomes.length); outcomes.push(o); } return seen.get(key); };
    const rows = cases.map((c) => {
        if (!kinds.includes(c.k)) kinds.push(c.k);
        return [kinds.indexOf(c.k), recipe(c.p, b.frame_len), c.u ? -1 : oidx(c.v), c.u ? -1 : oidx(c.n)];
    });
    return JSON.stringify({ ...head, kinds, outcomes, cases: rows });
}).join(',\n');
s += '\n]}\n';
fs.writeFileSync(path.join(OUT, 'damaged_frames.json'), s);
console.log('wrote', doc.bases.reduce((a, b) => a + b.cases.length, 0), 'cases to', path.join(OUT, 'damaged_frames.json'));
}
main().catch((e) => { console.error(e); process.exit(1); });
