// tools/golden/gen_enc_shapes.mjs — records what the reference's compressBlock writes for the encoder
// shapes of tests/enc_shapes_common.py, by EXECUTING the reference JavaScript. Run:
//   (cd tests && python -c "import conftest, enc_shapes_common as E; E.dump('<scratch dir>')")
//   node tools/golden/gen_enc_shapes.mjs <checkout of the reference> <scratch dir> tests/golden
// It writes tests/golden/enc_shapes.json and nothing else.
//
// This script contains only harness code. It imports the reference modules by absolute path at run
// time; nothing of the reference is copied. The inputs are the cases Python dumped (cases.json and one
// file per distinct source and table); the fixture holds digests only, no source bytes. Per case:
//   [XXH32 of the source, XXH32 of the initial table (little-endian int32 x 16384),
//    the length of each block's output, XXH32 over the blocks' XXH32s (little-endian u32s in order),
//    XXH32 of the final table]
// where the blocks are compressBlock(src, scratch, start_b, n_b, table, 0) in order with one carried
// Int32Array(16384) (bufferCompress.js's loop), or one call over [start, start + len) when the case has
// no block size.
import fs from 'fs';
import path from 'path';

const REF = process.argv[2];
const IN = process.argv[3];
const OUT = process.argv[4] || 'tests/golden';
if (!REF || !IN) { console.error('usage: node tools/golden/gen_enc_shapes.mjs <checkout of the reference> <dumped cases> [tests/golden]'); process.exit(2); }

const hex = (h) => (h >>> 0).toString(16).padStart(8, '0');
const bytesOf = (i32) => new Uint8Array(i32.buffer, i32.byteOffset, i32.byteLength);

async function main() {
    const { compressBlock } = await import(path.join(REF, 'src/block/blockCompress.js'));
    const { xxHash32 } = await import(path.join(REF, 'src/xxhash32/xxhash32.js'));
    const files = new Map();
    const load = (name) => {
        if (!files.has(name)) files.set(name, new Uint8Array(fs.readFileSync(path.join(IN, name))));
        return files.get(name);
    };
    const cases = JSON.parse(fs.readFileSync(path.join(IN, 'cases.json'), 'utf8'));
    const lines = [];
    for (const c of cases) {
        const src = load(c.src);
        const table = new Int32Array(16384);
        if (c.table) table.set(new Int32Array(load(c.table).slice().buffer));
        const tableXxh = hex(xxHash32(bytesOf(table), 0));
        const sizes = [];
        if (c.block_size === null) sizes.push(c.len);
        else for (let p = 0; p < c.len; p += c.block_size) sizes.push(Math.min(c.block_size, c.len - p));
        const lens = [];
        const digests = new Uint32Array(sizes.length);
        let pos = c.start;
        sizes.forEach((n, b) => {
            const scratch = new Uint8Array(n + Math.floor(n / 255) + 16);
            const w = compressBlock(src, scratch, pos, n, table, 0);
            lens.push(w);
            digests[b] = xxHash32(scratch.subarray(0, w), 0) >>> 0;
            pos += n;
        });
        const row = [hex(xxHash32(src, 0)), tableXxh, lens, hex(xxHash32(bytesOf(digests), 0)), hex(xxHash32(bytesOf(table), 0))];
        lines.push(' ' + JSON.stringify(c.name) + ': ' + JSON.stringify(row));
    }
    const head = { generator: 'tools/golden/gen_enc_shapes.mjs',
                   what: "the reference's compressBlock on the cases of tests/enc_shapes_common.py: digests only" };
    const doc = '{\n "generator": ' + JSON.stringify(head.generator) + ',\n "what": ' + JSON.stringify(head.what) +
                ',\n "cases": {\n' + lines.join(',\n') + '\n }\n}\n';
    fs.writeFileSync(path.join(OUT, 'enc_shapes.json'), doc);
    console.log('wrote', lines.length, 'cases,', doc.length, 'bytes');
}
main();
