// tools/golden/gen_linked_exact.mjs — records what the reference's decompressBlock leaves in ONE output
// array when the blocks of a batch are decoded in index order, by EXECUTING the reference JavaScript.
// Run:
//   node tools/golden/gen_linked_exact.mjs <checkout of the reference> tests/golden
// It writes tests/golden/linked_exact.json and nothing else (manifest.json is gen_golden.mjs's).
//
// This script contains only our own hand-assembled blocks and harness code. It imports the reference
// module by absolute path at run time; nothing of the reference is copied.
//
// The cases pin LZ4MI_LINKED_EXACT (include/lz4mi.h): the reference's double-copy-tail rewrite of a
// match with offset >= 8 and length < 8 (blockDecompress.js:219-250) at a block's FIRST sequence
// reaches below the block's start, into the block before it or the caller's bytes. Per case: the
// blocks (hex; `stored`: raw bytes the frame layer copies, bufferDecompress.js:173-180), the slots
// (out_off, out_cap: a call sees the array up to its slot's end, the capacity of a one-block call),
// the initial array, an optional dictionary, the array afterwards and each call's return value or
// error message.
import fs from 'fs';
import path from 'path';

const REF = process.argv[2];
const OUT = process.argv[3] || 'tests/golden';
if (!REF) { console.error('usage: node tools/golden/gen_linked_exact.mjs <checkout of the reference> [tests/golden]'); process.exit(2); }

const hex = (b) => Buffer.from(b).toString('hex');
// distinct, non-zero bytes: a rewrite that lands anywhere else shows
const ramp = (n, from) => Array.from({ length: n }, (_, k) => ((from + 7 * k) % 251) + 1);

// One LZ4 sequence: literals, then (off, ml) unless off is 0 (the block's last sequence).
function seq(lits, off = 0, ml = 0) {
    const o = [];
    const ll = lits.length;
    const mcode = off ? ml - 4 : 0;
    o.push((Math.min(ll, 15) << 4) | Math.min(mcode, 15));
    if (ll >= 15) { let r = ll - 15; while (r >= 255) { o.push(255); r -= 255; } o.push(r); }
    o.push(...lits);
    if (off) {
        o.push(off & 255, off >> 8);
        if (mcode >= 15) { let r = mcode - 15; while (r >= 255) { o.push(255); r -= 255; } o.push(r); }
    }
    return o;
}
const block = (...seqs) => Uint8Array.from(seqs.flat());
const tail5 = (from) => seq(ramp(5, from));

// back to back slots of the given decoded sizes
function backToBack(sizes, first = 0) {
    const off = []; let p = first;
    for (const n of sizes) { off.push(p); p += n; }
    return off;
}

function cases() {
    const L32 = block(seq(ramp(32, 10)));                       // 32 literal bytes
    const first = (ll, off, ml, from) => block(seq(ramp(ll, from), off, ml), tail5(from + 90));   // ll + ml + 5 bytes
    const c = [];
    const add = (name, blocks, sizes, extra = {}) => {
        const out_off = extra.out_off || backToBack(sizes, extra.first || 0);
        const out_cap = extra.out_cap || sizes;
        const total = extra.total || out_off[out_off.length - 1] + out_cap[out_cap.length - 1];
        c.push({ name, note: extra.note || '', blocks, out_off, out_cap, init: Uint8Array.from(ramp(total, 200)),
                 dict: extra.dict || null });
    };
    const B = (bytes, stored = false) => ({ bytes, stored });
    add('ll0_ml4_off8', [B(L32), B(first(0, 8, 4, 50))], [32, 9], { note: '4 bytes into the predecessor' });
    add('ll3_ml4_off8', [B(L32), B(first(3, 8, 4, 50))], [32, 12], { note: '1 byte into the predecessor, 3 literals rewritten' });
    add('ll0_ml7_off9', [B(L32), B(first(0, 9, 7, 50))], [32, 12], { note: '1 byte into the predecessor' });
    add('ll4_ml4_control', [B(L32), B(first(4, 8, 4, 50))], [32, 13], { note: 'control: the region starts at the block' });
    add('rewritten_source', [B(L32), B(block(seq([], 8, 4), seq(ramp(8, 60)))), B(first(0, 12, 4, 70))], [32, 12, 9],
        { note: "block 2's rewrite reads the bytes block 1's rewrite changed" });
    add('pred_overlap_off1', [B(block(seq(ramp(8, 10), 1, 20))), B(first(0, 24, 4, 50))], [28, 9],
        { note: 'the predecessor ends in a run (offset 1) that covers the region' });
    add('pred_overlap_off2', [B(block(seq(ramp(10, 10), 2, 18))), B(first(0, 24, 4, 50))], [28, 9],
        { note: 'the predecessor ends in a period-2 match that covers the region' });
    for (const n of [1, 2, 3])
        add('tiny_pred_' + n, [B(L32), B(block(seq(ramp(n, 40)))), B(first(0, 8, 4, 50)), B(first(1, 16, 5, 80))],
            [32, n, 9, 11], { note: 'the region spans two boundaries' });
    add('stored_pred', [B(L32), B(Uint8Array.from(ramp(16, 120)), true), B(first(0, 8, 4, 50)), B(first(0, 10, 5, 80))],
        [32, 16, 9, 10], { note: 'the predecessor is a stored block' });
    add('gap', [B(L32), B(first(0, 8, 4, 50)), B(first(2, 8, 4, 80))], [32, 9, 11],
        { out_off: [0, 38, 47], note: "6 of the caller's bytes between the slots" });
    add('short_tail', [B(L32), B(first(0, 8, 4, 50)), B(first(0, 11, 6, 80))], [32, 9, 11],
        { out_off: [0, 40, 49], out_cap: [40, 9, 11], note: 'the first slot has 8 unused bytes' });
    add('first_over_history', [B(first(0, 8, 4, 50)), B(first(0, 8, 4, 80))], [9, 9],
        { first: 20, note: "the call's first block rewrites the caller's bytes before it" });
    add('first_at_0', [B(block(seq(ramp(8, 10), 8, 4), tail5(100))), B(first(0, 8, 4, 50))], [17, 9],
        { note: 'the rewrite reads before the array: 0' });
    add('first_at_0_dict', [B(block(seq(ramp(8, 10), 8, 4), tail5(100))), B(first(0, 8, 4, 50))], [17, 9],
        { dict: Uint8Array.from(ramp(16, 150)), note: 'the same with a dictionary: still 0, not a dictionary byte' });
    add('dict_match_then_rewrite', [B(block(seq(ramp(2, 10), 6, 8), seq(ramp(3, 30), 9, 4), tail5(100))), B(first(0, 8, 4, 50))],
        [22, 9], { dict: Uint8Array.from(ramp(16, 150)), note: 'a match out of the dictionary, then rewrites' });
    return c;
}

async function main() {
    const { decompressBlock } = await import(path.join(REF, 'src/block/blockDecompress.js'));
    const out = [];
    for (const c of cases()) {
        const arr = Uint8Array.from(c.init);
        const results = [];
        c.blocks.forEach((b, k) => {
            const off = c.out_off[k], cap = c.out_cap[k];
            if (b.stored) {
                arr.set(b.bytes, off);                        // bufferDecompress.js:173-180
                results.push(b.bytes.length);
                return;
            }
            try {
                results.push(decompressBlock(b.bytes, 0, b.bytes.length, arr.subarray(0, off + cap), off, c.dict || undefined));
            } catch (e) {
                results.push(String(e.message));
            }
        });
        out.push({ name: c.name, note: c.note, blocks: c.blocks.map((b) => hex(b.bytes)), stored: c.blocks.map((b) => b.stored),
                   out_off: c.out_off, out_cap: c.out_cap, init: hex(c.init), dict: c.dict ? hex(c.dict) : null,
                   after: hex(arr), results });
    }
    const doc = { generator: 'tools/golden/gen_linked_exact.mjs',
                  what: "the reference's decompressBlock on the blocks in index order on one array", cases: out };
    fs.writeFileSync(path.join(OUT, 'linked_exact.json'), JSON.stringify(doc, null, 1) + '\n');
    console.log('wrote', out.length, 'cases');
}
main();
