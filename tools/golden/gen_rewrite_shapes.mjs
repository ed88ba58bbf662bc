// tools/golden/gen_rewrite_shapes.mjs — records what the reference's decompressBlock leaves for the built
// blocks of tests/rewrite_shapes_common.py, by EXECUTING the reference JavaScript. Run:
//   (cd tests && python -c "import conftest, rewrite_shapes_common as X; X.dump('<scratch dir>')")
//   node tools/golden/gen_rewrite_shapes.mjs <checkout of the reference> <scratch dir> tests/golden
// It writes tests/golden/rewrite_shapes.json and nothing else.
//
// This script contains only harness code. It imports the reference modules by absolute path at run
// time; nothing of the reference is copied. The inputs are the shapes Python dumped (shapes.json and one
// file per distinct block, history and dictionary); the fixture holds digests only. Per shape:
//   [XXH32 of the block, the bytes written or the error's message, XXH32 of the whole array afterwards]
// where the array is the history followed by `cap` zero bytes and the call is
// decompressBlock(block, 0, block.length, array, history.length, dictionary).
import fs from 'fs';
import path from 'path';

const REF = process.argv[2];
const IN = process.argv[3];
const OUT = process.argv[4] || 'tests/golden';
if (!REF || !IN) { console.error('usage: node tools/golden/gen_rewrite_shapes.mjs <checkout of the reference> <dumped shapes> [tests/golden]'); process.exit(2); }

const hex = (h) => (h >>> 0).toString(16).padStart(8, '0');

async function main() {
    const { decompressBlock } = await import(path.join(REF, 'src/block/blockDecompress.js'));
    const { xxHash32 } = await import(path.join(REF, 'src/xxhash32/xxhash32.js'));
    const load = (name) => new Uint8Array(fs.readFileSync(path.join(IN, name)));
    const shapes = JSON.parse(fs.readFileSync(path.join(IN, 'shapes.json'), 'utf8'));
    const lines = [];
    for (const s of shapes) {
        const comp = load(s.comp);
        const out = new Uint8Array(s.out_off + s.cap);
        if (s.history) out.set(load(s.history));
        const dict = s.dictionary ? load(s.dictionary) : undefined;
        let result;
        try {
            result = decompressBlock(comp, 0, comp.length, out, s.out_off, dict);
        } catch (e) {
            result = e.message;
        }
        const row = [hex(xxHash32(comp, 0)), result, hex(xxHash32(out, 0))];
        lines.push(' ' + JSON.stringify(s.name) + ': ' + JSON.stringify(row));
    }
    const doc = '{\n "generator": "tools/golden/gen_rewrite_shapes.mjs",\n "what": ' +
                JSON.stringify("the reference's decompressBlock on the shapes of tests/rewrite_shapes_common.py: digests only") +
                ',\n "shapes": {\n' + lines.join(',\n') + '\n }\n}\n';
    fs.writeFileSync(path.join(OUT, 'rewrite_shapes.json'), doc);
    console.log('wrote', lines.length, 'shapes,', doc.length, 'bytes');
}
main();
