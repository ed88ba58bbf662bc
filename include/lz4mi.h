/*
 * include/lz4mi.h — C-ABI of the MI355X-native LZ4 block codec (liblz4mi.so).
 *
 * This is the drop-in boundary the reference's hot path is re-bound to. Each
 * entry point names the reference interface it replaces (paths relative to the
 * divortio-lz4 repository root). The N-API addon (divortio-lz4_amd/napi/) and
 * the Python ctypes binding (divortio-lz4_amd/lz4mi/) are thin shims over it.
 *
 * Conventions
 *  - Plain pointers and sizes; no framework types.
 *  - By default every pointer is HOST memory: the call stages it to the GPU,
 *    runs the kernel and copies results back before returning (synchronous,
 *    like the reference's functions).
 *  - With LZ4MI_DEVICE_PTRS every pointer (data AND the per-block descriptor
 *    arrays) is DEVICE memory, the call only enqueues work on `stream`
 *    (a hipStream_t; NULL = HIP's default stream) and returns without waiting
 *    for the device or reading anything back; status/out_len are valid once the
 *    stream has been synchronised. Scratch memory is per stream, so calls on
 *    different streams may run concurrently.
 *  - Status codes: 0 = OK, negative = the reference's error (one per message,
 *    see lz4mi_status_message), <= -100 = infrastructure failure.
 */
#ifndef LZ4MI_H
#define LZ4MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (per block / per call) ------------------------------- */
#define LZ4MI_OK 0
#define LZ4MI_ERR_OUTPUT_TOO_SMALL (-1) /* "LZ4: Output Buffer Too Small"  src/block/blockDecompress.js:74 */
#define LZ4MI_ERR_MALFORMED (-2)        /* "LZ4: Malformed Input"          src/block/blockDecompress.js:75 */
#define LZ4MI_ERR_OFFSET0 (-3)          /* "LZ4: Invalid Offset 0"         src/block/blockDecompress.js:128 */
#define LZ4MI_ERR_DICT_OOB (-4)         /* "LZ4: Dictionary Offset Out of Bounds" src/block/blockDecompress.js:150-152 */
#define LZ4MI_ERR_MAGIC (-5)            /* "LZ4: Invalid Magic Number"     src/buffer/bufferDecompress.js:60 */
#define LZ4MI_ERR_VERSION (-6)          /* "LZ4: Unsupported Version v"    src/buffer/bufferDecompress.js:67 */
#define LZ4MI_ERR_CHECKSUM (-7)         /* "LZ4: Content Checksum Error"   src/buffer/bufferDecompress.js:216 */
#define LZ4MI_ERR_RANGE (-8)            /* RangeError "Source is too large" of TypedArray.set: a literal run
                                           > 64 bytes that does not fit `output` (blockCompress.js:100,198),
                                           a stored block past the result (bufferDecompress.js) */
#define LZ4MI_ERR_CROSS_BLOCK (-9)      /* batched decode only: a back-reference reaches before the block's
                                           own output (not an independent block); the frame layer then
                                           decodes the frame's blocks in order, one call per block */
#define LZ4MI_ERR_BLOCK_CHECKSUM (-10)  /* a frame block's checksum (FLG bit 0x10) does not match its payload;
                                           reported only when block-checksum verification is asked for (the
                                           reference skips them: src/buffer/bufferDecompress.js:191) */
#define LZ4MI_ERR_HIP (-100)            /* a HIP runtime call failed */
#define LZ4MI_ERR_ARG (-101)            /* invalid argument (size limits, NULL pointers) */
#define LZ4MI_ERR_NO_DEVICE (-102)      /* no usable gfx950 device */
#define LZ4MI_ERR_DEVICE_BOUND (-103)   /* lz4mi_init(d): the library is already bound to another device (one
                                           device per process: its stream and scratch live on the first) */

/* ---- flags --------------------------------------------------------------- */
#define LZ4MI_DEVICE_PTRS 0x1u   /* all pointers are device pointers; async on `stream` */
#define LZ4MI_JS_COMPAT 0x2u     /* decode exactly like the reference JS decoder, including its
                                    double-copy-tail rewrite. Default: LZ4 spec. */
#define LZ4MI_XXH_STANDARD 0x4u  /* spec XXH32 lane convergence instead of the reference's variant */
#define LZ4MI_JS_EXACT 0x8u      /* reference-exact result at spec-decoder speed: blocks are decoded by the
                                    parallel spec kernel, which checks every 1 KiB chunk for a reference
                                    double-copy-tail rewrite (F1) that would change a byte and, only in such
                                    a chunk, replays the chunk's matches with the reference's semantics
                                    before going on (cost proportional to the affected chunks). */

#define LZ4MI_XXH_LEN64 0x10u    /* streaming XXH32: keep the 64-bit total length (streams over 2 GiB);
                                    default: the reference class's `(totalLen + len) | 0` */
#define LZ4MI_BLOCK_CHECKSUM 0x20u /* lz4mi_frame_pack: records carry XXH32 (spec) of their payload (FLG 0x10) */
#define LZ4MI_FRAME_WORDS 0x40u  /* lz4mi_decompress_blocks (device pointers, not with LZ4MI_JS_COMPAT): in_len[b]
                                    is the frame's raw size word; bit 31 set = a stored block, whose bytes are
                                    copied in the same launch (bufferDecompress.js:173-180: LZ4MI_ERR_RANGE when
                                    they exceed out_cap[b], the reference's result.set RangeError) */
#define LZ4MI_LINKED 0x80u       /* lz4mi_decompress_blocks, lz4mi_frame_decompress (spec mode): the blocks may
                                    reference the output of the blocks before them (dependent-block frames);
                                    the whole batch is decoded in one call. Contract: lz4mi_decompress_blocks.
                                    The reference decoder's bytes for such a batch: LZ4MI_LINKED_EXACT. */
#define LZ4MI_LINKED_EXACT 0x100u /* lz4mi_decompress_blocks, lz4mi_frame_decompress: LZ4MI_LINKED with the result
                                    of the reference decoder run on the blocks in order on one array, its
                                    double-copy-tail rewrite (F1) across block boundaries included. Implies
                                    LZ4MI_LINKED. Contract: lz4mi_decompress_blocks. */
#define LZ4MI_VERIFY_BLOCKS 0x200u /* lz4mi_frame_decompress: check the frame's block checksums (FLG 0x10) on the
                                    device, lz4mi_verify_blocks over the frame's payloads; a mismatch is the
                                    frame's error LZ4MI_ERR_BLOCK_CHECKSUM. No effect on a frame without them. */
#define LZ4MI_VERIFY_CONTENT 0x400u /* lz4mi_frames_decompress: check every decoded frame's content checksum (FLG 0x04)
                                    on the device, one XXH32 chain (the reference's variant) per frame, all frames
                                    in one launch; a mismatch is that frame's error LZ4MI_ERR_CHECKSUM. */
#define LZ4MI_FRAMES_MEASURE 0x800u /* lz4mi_frames_index: measure every frame's block sizes (lz4mi_decoded_sizes),
                                    also where a content size would give them from the reference encoder's layout:
                                    for frames with partial blocks in the middle. */
/* lz4mi_frames_plan / lz4mi_frames_compress (and their host twins): */
#define LZ4MI_FRAMES_CONTENT_CHECKSUM 0x1000u /* FLG 0x04: the reference's XXH32 variant of the source behind the EndMark */
#define LZ4MI_FRAMES_NO_CONTENT_SIZE 0x2000u  /* leave the content size field out (default: written, like the reference) */
#define LZ4MI_FRAMES_DEPENDENT 0x4000u        /* FLG without 0x20 (the reference's default): frames of at most one block,
                                                 with LZ4MI_FRAMES_CHAINS also the longer ones */
#define LZ4MI_FRAMES_PACKED 0x8000u           /* lz4mi_frames_compress: the frames back to back from out[0] */
#define LZ4MI_FRAMES_CHAINS 0x10000u          /* with LZ4MI_FRAMES_DEPENDENT (alone: LZ4MI_ERR_ARG): a frame of more than
                                                 one block is listed and written too, its blocks encoded in order with
                                                 one table carried across them, one chain per frame, all chains at once.
                                                 lz4mi_frames_decompress: frames whose blocks read the blocks before
                                                 them are decoded in the call, one wave per frame in block order,
                                                 instead of being declined (contract there) */

/* ---- why lz4mi_frames_index / lz4mi_frames_decompress (and lz4mi_frames_plan / lz4mi_frames_compress) leave a
 *      frame to the caller (finfo[f][7]) ---- */
#define LZ4MI_FRAMES_DECLINE_CAP_BLOCKS 1    /* its blocks are not in the lists: cap_blocks (nblocks) too small */
#define LZ4MI_FRAMES_DECLINE_PAST_END 2      /* the walk of its size words ran past the frame's end (a cut frame) */
#define LZ4MI_FRAMES_DECLINE_EMPTY 3         /* no blocks, or the content-size flag with size 0 (the empty frame) */
#define LZ4MI_FRAMES_DECLINE_UNSIZED_EXACT 4 /* no content size, with LZ4MI_JS_EXACT: the reference decodes such a frame
                                                behind a window, where its tail rewrite lands elsewhere */
#define LZ4MI_FRAMES_DECLINE_MEASURE 5       /* a measured block fails the size walk, or a frame without a content size
                                                has a compressed block above its block_max */
#define LZ4MI_FRAMES_DECLINE_SIZE_MISMATCH 6 /* the measured total differs from the content size */
#define LZ4MI_FRAMES_DECLINE_OUT_CAP 7       /* the decoded total is above frame_out_cap[f] */
#define LZ4MI_FRAMES_DECLINE_LAYOUT 8        /* not the reference encoder's layout (a compressed block other than the last
                                                that does not fill its slot: where lz4mi_frame_decompress returns
                                                LZ4MI_ERR_ARG); a measured frame with a failing block */
#define LZ4MI_FRAMES_DECLINE_DEPENDENT 9     /* a block reads the output of the block before it (LZ4MI_ERR_CROSS_BLOCK);
                                                with LZ4MI_JS_EXACT also block 0's tail rewrite reading below the frame */
#define LZ4MI_FRAMES_DECLINE_HASH_4G 10      /* LZ4MI_VERIFY_CONTENT and a result of 4 GiB or more */

/* Largest block the kernels accept (the reference's largest block size is 4 MiB;
 * raw calls may pass more, up to 2^31-1 like the reference's `|0` arithmetic).
 * The limit is exercised by tests/test_gpu_big_blocks.py: blocks of 128 MiB to 2^31-1
 * bytes through the decoder and the size pass, blocks of up to 40 MiB through the encoder. */
#define LZ4MI_MAX_BLOCK 0x7FFFFFFFu

/* Worst-case compressed size of an n-byte block (n + n/255 + 16). */
static inline uint64_t lz4mi_compress_bound(uint64_t n) { return n + n / 255u + 16u; }

/* Human-readable message of a status (the reference's exact error string). */
const char* lz4mi_status_message(int32_t status);

/* Device selection / info. Returns LZ4MI_OK or LZ4MI_ERR_*. lz4mi_init(-1) keeps the
 * current device (or HIP's current one). The library binds to one device per process (one
 * process per GPU): asking for another device once initialised returns LZ4MI_ERR_ARG. */
int32_t lz4mi_init(int32_t device);
int32_t lz4mi_device_count(void);
const char* lz4mi_version(void);
/* Hash of the sources the library was compiled from (Makefile SRC_HASH): lets a test
 * prove the loaded binary was built from the tree beside it. */
const char* lz4mi_build_id(void);

/*
 * Batched raw-block DECOMPRESS.
 * Replaces: decompressBlock(input, inputOffset, inputSize, output, outputOffset, dictionary)
 *           src/block/blockDecompress.js:30-275 (exported as LZ4.decompressRaw, src/lz4.js:33),
 *           and the per-block loop of decompressBuffer src/buffer/bufferDecompress.js:133-192.
 * Block b reads in[in_off[b] .. +in_len[b]) and writes out[out_off[b] ..
 * +out_cap[b]). Positions are absolute in `out` exactly as in the reference:
 * a back-reference below out[out_off[b]] reads earlier bytes of `out`, and
 * below out[0] reads the tail of `dict` (dict_len bytes, may be 0).
 * out_len[b] = bytes produced (outPos - outputOffset); status[b] per block.
 * With nblocks > 1 the blocks must be independent: a back-reference that
 * reaches before the block's own output start yields LZ4MI_ERR_CROSS_BLOCK
 * for that block (with nblocks == 1 it reads the preceding bytes of `out`,
 * then `dict`, exactly as the reference). LZ4MI_JS_COMPAT decodes the blocks
 * in order on one lane with the reference's byte-level behaviour.
 * Returns LZ4MI_OK when the batch ran (per-block errors are in status[]).
 * Footprint (tests/test_gpu_footprint.py): a block with status 0 writes out[out_off[b] .. +min(out_len[b],
 * out_cap[b])) and nothing else -- the rest of its slot, the bytes around it, `in`, and the entries of
 * out_len[] / status[] from nblocks on stay the caller's; a match that is the block's last sequence is
 * clipped at the capacity like a store to a typed array and gives status 0 with out_len[b] > out_cap[b].
 * Only a lone block (nblocks == 1) in a reference mode also rewrites up to 4 bytes below its slot (the
 * reference's tail rewrite of its first sequence), and LZ4MI_LINKED_EXACT as described below. A block
 * with status != 0 has out_len[b] = 0 and may have written inside its own slot only (not the
 * reference's partial output); a stored block that does not fit (LZ4MI_ERR_RANGE) writes nothing.
 *
 * LZ4MI_LINKED (spec mode; with LZ4MI_JS_COMPAT or LZ4MI_JS_EXACT: LZ4MI_ERR_ARG; the reference
 * decoder's bytes: LZ4MI_LINKED_EXACT, below): dependent blocks
 * in one call. Precondition: the output slots are ascending and disjoint, out_off[b] + out_cap[b]
 * <= out_off[b+1]; gaps are allowed, the caller's bytes there are final. Result: the bytes,
 * out_len[] and status[] that nblocks successive nblocks == 1 calls in index order on the same
 * `out` would give: a back-reference below a block's start reads the earlier block's freshly
 * decoded bytes where it falls inside an earlier slot of the batch (up to that block's out_len),
 * the caller's bytes of `out` otherwise, and the tail of `dict` below out[0]. The capacity,
 * dictionary-bounds and other checks keep their absolute-position meaning; LZ4MI_ERR_CROSS_BLOCK is
 * not a check here. After a failure: the first block in index order with status != 0 keeps it;
 * every later block gets LZ4MI_ERR_CROSS_BLOCK, out_len 0 and is not written (the caller can resume
 * from the failing block). Limits: out_cap[b] <= 4 MiB and in_len[b] <= lz4mi_compress_bound(4 MiB);
 * a block past them, or a slot that breaks the precondition, is LZ4MI_ERR_ARG for the call with
 * host pointers and status LZ4MI_ERR_ARG for that block (then the after-failure rule) with device
 * pointers -- as is a block of a device-pointer batch whose slots are spread so far that a pass
 * cannot address them. The rule, per pass (at most ~240 blocks of 4 MiB), with in_lo / out_lo the
 * lowest in_off / out_off of the pass's blocks: block b is refused when
 *     in_off[b] - in_lo + in_len[b] >= 2^30   or   out_off[b] - out_lo + out_cap[b] + 65536 >= 2^30
 * (in_len without the stored bit of a frame word; the lowest slot itself counts, so one block
 * always fits). One byte less in either sum decodes. Valid with
 * LZ4MI_DEVICE_PTRS (asynchronous, nothing read back) and with host pointers (the whole output range
 * is staged: gaps and unused slot tails are history); with LZ4MI_FRAME_WORDS on device pointers a
 * stored block is copied in the same call before anything reads it. Any nblocks: the call cuts the
 * batch into passes in index order on the one stream, as many blocks each as the scratch cap
 * (LZ4MI_SMALL_SCRATCH_MB, compared with the real allocation) and the pointer encodings allow.
 *
 * LZ4MI_LINKED_EXACT (implies LZ4MI_LINKED, setting both changes nothing; with LZ4MI_JS_COMPAT or
 * LZ4MI_JS_EXACT: LZ4MI_ERR_ARG): a linked batch in the reference decoder's bytes. Result: the bytes,
 * out_len[] and status[] of nblocks successive one-block LZ4MI_JS_EXACT calls in index order on the
 * caller's array. The reference's tail rewrite of a match at absolute position s with offset >= 8 and
 * length ml < 8 (blockDecompress.js:219-250) sets out[p] = out[p - off] for p in [s + ml - 8, s); at a
 * block's first sequence with fewer than 8 - ml literals that region lies below the block's own start,
 * in the tail of the block before it or in the caller's bytes, and is rewritten there (host pointers:
 * the up to 8 bytes below every decoded block are copied back with it). LZ4MI_LINKED's rules for
 * slots, the 4 MiB limits, LZ4MI_FRAME_WORDS, passes and failures hold; the first failing block and
 * every block after it write nothing, a rewrite below their own slot included. Refusal: a block
 * whose region below its start touches a byte that is not the decoded output of an earlier block of
 * the same pass (a gap, a stored block, the unused tail of a short slot) while the block is not the
 * first of its pass, or whose rewrite would read below out[0] with a dictionary present, gets
 * LZ4MI_ERR_CROSS_BLOCK and the after-failure rule applies: decode that block alone with
 * LZ4MI_JS_EXACT and issue a new call for the blocks after it (lz4mi_frame_decompress does). A region
 * inside earlier blocks' decoded output, and the first block of the call (over the caller's bytes;
 * positions below out[0] are not written and read as 0), always decode in the call.
 */
int32_t lz4mi_decompress_blocks(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                                uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap,
                                const uint8_t* dict, uint32_t dict_len,
                                uint32_t* out_len, int32_t* status, uint32_t nblocks, uint32_t flags,
                                void* stream);

/*
 * Batched DECODED SIZES of raw blocks, without decoding them.
 * Replaces nothing the reference exports: it is the sequence walk of decompressBlock,
 *           src/block/blockDecompress.js:55-139, with every copy left out, for callers that hold
 *           blocks without their decoded lengths (frames without a content size or with partial
 *           blocks, src/buffer/bufferDecompress.js:104-131).
 * out_len[b] = the sum of the literal and match lengths along block b's token chain, i.e.
 * outPos - outputOffset where the reference's loop ends or throws; status[b] = the first error, in
 * sequence order, of the two that do not depend on output positions: LZ4MI_ERR_MALFORMED (:75) and
 * LZ4MI_ERR_OFFSET0 (:128), Malformed tested first within a sequence. Output Buffer Too Small,
 * Dictionary Offset Out of Bounds and LZ4MI_ERR_CROSS_BLOCK depend on where the output lies and
 * are not detected here (the walk goes on). Lengths accumulate in 64 bits: a total above
 * LZ4MI_MAX_BLOCK gives LZ4MI_ERR_OUTPUT_TOO_SMALL with out_len[b] = 0x7FFFFFFF (no decode call
 * could be given such a capacity). in_len[b] == 0: size 0, status 0. Bytes past a block's end
 * read as 0 (the reference's `undefined | 0`): nothing outside in[in_off[b] .. +in_len[b]) is read.
 * flags: LZ4MI_DEVICE_PTRS (asynchronous on `stream`, no scratch, nothing read back);
 * LZ4MI_FRAME_WORDS (in_len[b] is a frame size word: bit 31 set = a stored block, size =
 * word & 0x7FFFFFFF, status 0). Any other flag: LZ4MI_ERR_ARG. One wave per block.
 */
int32_t lz4mi_decoded_sizes(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                            uint32_t* out_len, int32_t* status, uint32_t nblocks,
                            uint32_t flags, void* stream);

/*
 * Batched raw-block COMPRESS (fresh hash table per block: independent blocks).
 * Replaces: compressBlock(src, output, srcStart, srcLen, hashTable, outputOffset)
 *           src/block/blockCompress.js:31-233 (LZ4.compressRaw, src/lz4.js:32) as called by
 *           compressBuffer's block loop src/buffer/bufferCompress.js:209-239 with
 *           blockIndependence=true. Output is byte-identical to the reference encoder.
 * Block b compresses in[in_off[b] .. +in_len[b]) into out[out_off[b] ..), a slot of
 * at least lz4mi_compress_bound(in_len[b]) bytes; out_len[b] = compressed size.
 * Footprint (tests/test_gpu_footprint.py): only out[out_off[b] .. +out_len[b]) and out_len[0 .. nblocks)
 * are written; the rest of a slot, up to its bound, stays the caller's.
 * The stored-block decision (bufferCompress.js:221-231) is the caller's.
 */
int32_t lz4mi_compress_blocks(const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len,
                              uint8_t* out, const uint64_t* out_off, uint32_t* out_len,
                              uint32_t nblocks, uint32_t flags, void* stream);

/*
 * Single raw-block COMPRESS with a caller-owned hash table (LZ4.compressRaw with any table).
 * Replaces: compressBlock src/block/blockCompress.js:31-233 with full semantics:
 * positions are absolute in src[0 .. src_total); the block is
 * src[src_start .. +src_len); `table` (16384 int32, values = position+1, <=0 empty)
 * is read and written back; output written at out[out_off ..) (out_total bytes
 * available in out; writes past it are dropped, as with a typed array).
 * With room for lz4mi_compress_bound(src_len) bytes at out_off the block runs on the GPU
 * (the dependent-chain kernel, one block, the table in LDS); with less, the reference's
 * RangeError of output.set() may interrupt the block, and the call runs the host encoder
 * (lz4mi_host_compress_block), which reproduces that store by store.
 * Returns the number of bytes the reference would report written (>= 0) or a
 * negative status (LZ4MI_ERR_RANGE: the reference threw; what it wrote before stays).
 */
int64_t lz4mi_compress_block_table(const uint8_t* src, uint64_t src_total, int32_t src_start, int32_t src_len,
                                   int32_t* table, uint8_t* out, uint64_t out_total, int32_t out_off,
                                   uint32_t flags, void* stream);

/*
 * XXH32, one buffer, on the host CPU (the frame content checksum is one serial
 * chain). Replaces: xxHash32(input, seed) src/xxhash32/xxhash32.js:21-98.
 * flags & LZ4MI_XXH_STANDARD selects the spec convergence.
 */
uint32_t lz4mi_xxh32(const uint8_t* data, size_t len, uint32_t seed, uint32_t flags);

/*
 * Streaming XXH32, on the host CPU.
 * Replaces: class XXHash32 src/xxhash32/xxhash32Stateful.js:13-152 — update() carries up to
 * 15 bytes between calls (:34-68); digest() (:110-152) does not change the state. The
 * length is kept as the class keeps it, `(totalLen + len) | 0` tested signed (:37, :113),
 * unless flags has LZ4MI_XXH_LEN64; LZ4MI_XXH_STANDARD selects the spec convergence.
 * The state is a plain 56-byte struct owned by the caller (no allocation).
 */
typedef struct lz4mi_xxh32_state {
    uint64_t opaque[7];
} lz4mi_xxh32_state;
void lz4mi_xxh32_reset(lz4mi_xxh32_state* state, uint32_t seed, uint32_t flags);
void lz4mi_xxh32_update(lz4mi_xxh32_state* state, const uint8_t* data, size_t len);
uint32_t lz4mi_xxh32_digest(const lz4mi_xxh32_state* state);

/*
 * Batched XXH32 of independent buffers on the GPU (per-block checksums,
 * dictionary ids, parity digests). hashes[b] = xxHash32(in[off[b] .. +len[b]), seed).
 */
int32_t lz4mi_xxh32_blocks(const uint8_t* in, const uint64_t* off, const uint32_t* len, uint32_t seed,
                           uint32_t* hashes, uint32_t nblocks, uint32_t flags, void* stream);

/*
 * Batched check of frame BLOCK CHECKSUMS on the GPU, in place.
 * Replaces nothing in the reference, whose reader skips them (src/buffer/bufferDecompress.js:191); it is the
 * check LZ4.decompress(..., verifyBlockChecksum) of the JS layer makes, without reading a hash back.
 * Record b is the payload in[in_off[b] .. +n) and the LE32 behind it, n = in_len[b]; status[b] = LZ4MI_OK when
 * that word equals XXH32 (spec convergence, seed 0) of the payload, else LZ4MI_ERR_BLOCK_CHECKSUM. in_total is
 * the size of `in`: nothing outside in[0 .. in_total) is read, and a record the end cuts (in_off[b] + n + 4 >
 * in_total) is LZ4MI_ERR_BLOCK_CHECKSUM without being hashed, as the JS layer reports it.
 * flags: LZ4MI_DEVICE_PTRS (asynchronous on `stream`, no scratch, nothing read back); LZ4MI_FRAME_WORDS
 * (in_len[b] is a frame size word: n = word & 0x7FFFFFFF; a stored block's payload is its raw bytes and is
 * hashed like any other). Any other flag: LZ4MI_ERR_ARG, as are a NULL status and NULL inputs with
 * nblocks > 0 (both before the device is looked at). With host pointers each whole record (payload + 4 bytes)
 * is staged, the kernel run and status[] copied back. One quad of lanes per record, as lz4mi_xxh32_blocks.
 * Footprint: only status[0 .. nblocks) is written.
 */
int32_t lz4mi_verify_blocks(const uint8_t* in, uint64_t in_total, const uint64_t* in_off, const uint32_t* in_len,
                            int32_t* status, uint32_t nblocks, uint32_t flags, void* stream);
/*
 * The same contract on the calling thread (host pointers, no device needed; flags: LZ4MI_FRAME_WORDS only):
 * the checker of the GPU pass, and what the host frame route uses.
 */
int32_t lz4mi_host_verify_blocks(const uint8_t* in, uint64_t in_total, const uint64_t* in_off, const uint32_t* in_len,
                                 int32_t* status, uint32_t nblocks, uint32_t flags);

/*
 * Frame block records on the device (independent-block frames).
 * Replaces the record writing of compressBuffer's block loop, src/buffer/bufferCompress.js:209-239:
 * block b's record goes to frame[rec_off[b] ..): LE32 comp_len[b] and the compressed bytes
 * comp[comp_off[b] ..) when 0 < comp_len[b] < raw_len[b], else LE32 (raw_len[b] | 0x80000000) and the
 * raw bytes raw[raw_off[b] ..). rec_off is the exclusive prefix sum of the record sizes (4 + payload).
 * flags & LZ4MI_BLOCK_CHECKSUM: each record ends with LE32 XXH32 (spec, seed 0) of its payload,
 * the block checksum of the LZ4 frame format (FLG bit 0x10; record size 8 + payload), which the
 * reference's reader skips (src/buffer/bufferDecompress.js:191) and its writer never emits.
 * Device pointers only (flags must include LZ4MI_DEVICE_PTRS); async on `stream`.
 */
int32_t lz4mi_frame_pack(const uint8_t* raw, const uint64_t* raw_off, const uint32_t* raw_len, const uint8_t* comp,
                         const uint64_t* comp_off, const uint32_t* comp_len, uint8_t* frame, const uint64_t* rec_off,
                         uint32_t nblocks, uint32_t flags, void* stream);

/*
 * LZ4 frame DECOMPRESS of a frame in device memory (content size present).
 * Replaces decompressBuffer src/buffer/bufferDecompress.js:51-220 ("direct write" strategy, :97):
 * the header and the size words are walked on the device (one lane: each record's position
 * depends on the previous size), stored blocks are copied (:146-148), and the compressed blocks
 * are decoded in one batch at the output positions of the reference encoder's layout; a block
 * that reads an earlier block's output (dependent frames) is then decoded alone, in order.
 * out: device buffer of out_cap >= content-size bytes. info (host, 8 x int64): [0] the reference's
 * error for the frame (first failing block in block order: LZ4MI_ERR_* of the block decoder,
 * LZ4MI_ERR_RANGE for a stored block past the content size, LZ4MI_ERR_MAGIC / _VERSION for the
 * header) or 0; [1] FLG; [2] content size; [3] bytes written; [4] stored blocks; [5] position
 * of the content checksum (after the EndMark) when FLG has 0x04; [6] block max size (BD).
 * The content checksum (one serial XXH32 chain) is the caller's to verify.
 * flags: LZ4MI_DEVICE_PTRS (required) | LZ4MI_JS_EXACT (reference-exact; default LZ4 spec)
 * | LZ4MI_LINKED (spec mode only, with LZ4MI_JS_EXACT: LZ4MI_ERR_ARG): the compressed blocks are
 * issued as one linked batch after the stored copies, so a dependent-block frame needs no launch
 * per block; without it dependent blocks are decoded one per launch, in order.
 * | LZ4MI_LINKED_EXACT (not with LZ4MI_JS_EXACT: LZ4MI_ERR_ARG): the same in the reference decoder's
 * bytes; a block the linked call refuses (the one after a stored block, usually) is decoded alone in
 * reference mode and the blocks after it go into a new linked call.
 * | LZ4MI_VERIFY_BLOCKS (with any of the above): on a frame with block checksums (FLG 0x10) the payloads of
 * both block lists are checked on the same stream (lz4mi_verify_blocks), the statuses read back with the
 * lists. Header errors and the frames this path does not take come first, as without the flag; then any
 * failing block checksum gives info[0] = LZ4MI_ERR_BLOCK_CHECKSUM, info[3] = 0 and LZ4MI_OK -- before the
 * layout checks on the decoded lengths (a damaged payload would fail them as LZ4MI_ERR_ARG) and before
 * every block's own error, a stored block's LZ4MI_ERR_RANGE included: all checksums are checked before a
 * block's result is looked at, the JS layer's rule. The decode launches may have run by then: the bytes of
 * out[0 .. content size) are unspecified, nothing outside them is written. Without FLG 0x10: no effect.
 * Synchronous (reads the header and the block lists back). Returns LZ4MI_ERR_ARG for frames
 * this path does not take (no content size, a block layout other than the reference encoder's,
 * out_cap too small): decode those with the host-buffer path block by block.
 */
int32_t lz4mi_frame_decompress(const uint8_t* frame, uint64_t len, uint8_t* out, uint64_t out_cap, int64_t* info,
                               uint32_t flags, void* stream);

/*
 * Dependent blocks of one frame (the reference's LZ4.compress default,
 * src/buffer/bufferCompress.js:182-236, which calls compressBlock once per block with one
 * table): block b = src[start + b*block_size, ...) compressed in order on one GPU chain with
 * `table` (Int32Array(16384) semantics, in/out, positions absolute in src) carried across
 * blocks; block b's bytes go to out + out_off[b] (room for lz4mi_compress_bound(n_b)),
 * comp_len[b] = its size, exactly compressBlock(src, scratch, start_b, n_b, table, 0). One
 * launch for the whole frame (one staging of src and the table). Host pointers only.
 */
int32_t lz4mi_compress_chain(const uint8_t* src, uint64_t src_total, int32_t start, int32_t len, int32_t block_size,
                             int32_t* table, uint8_t* out, const uint64_t* out_off, uint32_t* comp_len, uint32_t flags,
                             void* stream);

/*
 * Host-CPU block encoder (the routing of SURVEY.md §8b: serial-chain calls run on the calling
 * thread). Same contract as lz4mi_compress_block_table / lz4mi_compress_chain (host pointers,
 * no device needed); byte-identical output and table. Used by the JS layer for dependent-block
 * frames (LZ4.compress's default) and a dictionary's first block, and by
 * lz4mi_compress_block_table when the output has less room than the worst case.
 */
int64_t lz4mi_host_compress_block(const uint8_t* src, uint64_t src_total, int32_t src_start, int32_t src_len,
                                  int32_t* table, uint8_t* out, uint64_t out_total, int32_t out_off);
int32_t lz4mi_host_compress_chain(const uint8_t* src, uint64_t src_total, int32_t start, int32_t len,
                                  int32_t block_size, int32_t* table, uint8_t* out, const uint64_t* out_off,
                                  uint32_t* comp_len);
/*
 * Host-CPU block decoder of the same routing: decompressBlock(input, inputOffset, inputSize,
 * output, outputOffset, dictionary) (src/block/blockDecompress.js:30-275) on the calling thread,
 * for blocks that read their predecessors' output (dependent-block frames, decoded in order).
 * in[0 .. in_total) is the whole input array, out[0 .. out_total) the whole output array
 * (positions absolute in it; below 0 the tail of dict). flags & (LZ4MI_JS_EXACT | LZ4MI_JS_COMPAT):
 * the reference's bytes, its double-copy-tail rewrite included; else LZ4 spec.
 * Returns bytes written (outPos - outputOffset) or a negative status with the reference's meaning.
 */
int64_t lz4mi_host_decompress_block(const uint8_t* in, uint64_t in_total, int64_t in_off, int64_t in_size,
                                    uint8_t* out, uint64_t out_total, int64_t out_off, const uint8_t* dict,
                                    uint32_t dict_len, uint32_t flags);
/*
 * Host-CPU decoded size of one block: the walk of lz4mi_decoded_sizes (src/block/blockDecompress.js:55-139
 * without the copies) on the calling thread, no device needed; the checker of the GPU size pass.
 * Positions as in lz4mi_host_decompress_block: in[0 .. in_total) is the whole input array, the block is
 * in[in_off .. +in_size). A length field read past the block's end but inside in_total sees the real
 * bytes, as in the reference; lz4mi_decoded_sizes has no in_total and reads zeros there (the two agree
 * when in_total == in_off + in_size). Returns the size (0x7FFFFFFF with *status =
 * LZ4MI_ERR_OUTPUT_TOO_SMALL above LZ4MI_MAX_BLOCK) and *status = 0 / LZ4MI_ERR_MALFORMED /
 * LZ4MI_ERR_OFFSET0, or LZ4MI_ERR_ARG (NULL status, negative positions).
 */
int64_t lz4mi_host_decoded_size(const uint8_t* in, uint64_t in_total, int64_t in_off,
                                int64_t in_size, int32_t* status);
/*
 * Where the reference's walk of a block stops reading: the position (in `in`) behind the last length
 * or offset byte that decompressBlock reads for the block in[in_off .. +in_size). A well-formed block
 * gives in_off + in_size or less. Above it the decoder has read bytes behind the block's end (an
 * offset's second byte, a length's continuation bytes), which in the reference are the array's real
 * bytes (zeros past in_total) but zeros for lz4mi_decompress_blocks, whose blocks end at in_len[b]:
 * the frame layer decodes such a block of a damaged frame with lz4mi_host_decompress_block.
 * Returns LZ4MI_ERR_ARG for negative positions.
 */
int64_t lz4mi_host_block_read_end(const uint8_t* in, uint64_t in_total, int64_t in_off, int64_t in_size);

/*
 * Block index of a device-resident frame, for decoding its blocks on several devices
 * (the block walk of bufferDecompress.js:133-192 without decoding): one lane walks the
 * header and the size words and writes, per block in frame order, the payload position
 * (pay_off) and the raw size word (size_word, bit 31 = stored). info (8 x int64, device)
 * as lz4mi_frame_decompress's, with [3] = blocks listed, [7] = 1 when the walk ran past
 * the frame or past cap_blocks. Past cap_blocks, [3] is cap_blocks, no entry behind it is
 * written, and [5] is the position behind the size word of the first block that did not
 * fit. Device pointers only (LZ4MI_DEVICE_PTRS); asynchronous
 * on `stream`. Replaces nothing in the reference (its frame loop is serial in one call).
 */
int32_t lz4mi_frame_index(const uint8_t* frame, uint64_t len, uint64_t* pay_off, uint32_t* size_word,
                          uint32_t cap_blocks, int64_t* info, uint32_t flags, void* stream);

/*
 * A BATCH OF FRAMES decoded on the device: index, then decompress. Device pointers only (LZ4MI_DEVICE_PTRS
 * required), asynchronous on `stream`, nothing is read back by either call.
 * Replaces decompressBuffer (src/buffer/bufferDecompress.js:51-220) called once per frame: frame f is
 * in[frame_off[f] .. +frame_len[f]) (any alignment; nothing outside these ranges is read). Only the walk inside a
 * frame is serial, so the frames walk in parallel, one lane each, and the blocks of all of them are decoded by
 * one LZ4MI_FRAME_WORDS batch launch.
 *
 * lz4mi_frames_index lists every frame's blocks in frame order, frame after frame: blk_in_off[b] (absolute in
 * `in`), blk_word[b] (the raw size word, bit 31 = stored), blk_frame[b], and blk_size[b], the decoded size the
 * block is given: for a frame with a content size > 0 the reference encoder's layout (a stored block its
 * declared size; a compressed block min(block_max, content size - position), position advancing by block_max),
 * for a frame without one -- with LZ4MI_FRAMES_MEASURE for every frame -- the size measured by
 * lz4mi_decoded_sizes. finfo[f] (8 x int64 per frame):
 *   [0] the frame's error in the reference's meaning, or 0: after the index call LZ4MI_ERR_MAGIC or
 *       LZ4MI_ERR_VERSION (checked in this order, before the size field, DictID and HC byte are skipped);
 *   [1] FLG | BD << 8; bit 16: the frame's sizes were measured; bits 32-63: the LE32 behind the EndMark when FLG
 *       has 0x04 (the content checksum; bytes the frame's end cuts read as 0). Mask before comparing: FLG is
 *       [1] & 0xFF, BD is ([1] >> 8) & 0xFF, and the value is negative when the checksum's top bit is set;
 *   [2] the content size; [3] the decoded total the frame needs in `out` (the content size, or the measured
 *   sum); [4] its first block in the lists; [5] the position behind the EndMark, relative to the frame;
 *   [6] its block count; [7] 0 = lz4mi_frames_decompress decodes this frame, else LZ4MI_FRAMES_DECLINE_*.
 * A declined frame is not an error of the call: the caller decodes it alone (lz4mi_frame_decompress or the
 * host path). A frame with [0] != 0 or a decline CAP_BLOCKS / PAST_END / EMPTY has no blocks in the lists; the
 * blocks of the frames that fit are listed without gaps, and a frame whose blocks do not fit cap_blocks lists
 * none. totals (4 x int64): [0] the blocks needed (call again with that cap_blocks if it is above cap_blocks),
 * [1] the blocks listed, [2] the sum of [3] over the frames that are neither declined nor in error, [3] the
 * number of declined frames.
 * flags: LZ4MI_DEVICE_PTRS | LZ4MI_FRAMES_MEASURE | LZ4MI_JS_EXACT (decides only the UNSIZED_EXACT decline). Any
 * other flag, a NULL finfo / totals, NULL inputs with nframes > 0 or NULL lists with cap_blocks > 0:
 * LZ4MI_ERR_ARG before the device is looked at.
 * Footprint: finfo[0 .. 8 nframes), totals[0 .. 4), and entries [0, totals[1]) of the four lists; nothing else.
 *
 * lz4mi_frames_decompress takes the lists and finfo as the index call left them (nblocks = cap_blocks or
 * totals[1]) and decodes every frame with finfo[f][0] == 0 and finfo[f][7] == 0 into out[frame_out_off[f] ..
 * +finfo[f][3]), provided that fits frame_out_cap[f]. Afterwards, per frame:
 *   [0] the reference's error for the frame, as lz4mi_frame_decompress reports it: the first failing block in
 *       block order (LZ4MI_ERR_* of the block decoder; LZ4MI_ERR_RANGE for a stored block past the content size;
 *       a back-reference of block 0 below the frame's start is LZ4MI_ERR_DICT_OOB: the frame has no dictionary
 *       and its result starts at position 0), or LZ4MI_ERR_CHECKSUM (LZ4MI_VERIFY_CONTENT);
 *   [3] the bytes written: the largest end, relative to the frame's slot and at most its total, of a block with
 *       status 0 -- lz4mi_frame_decompress's info[3], with one difference: a stored block that fails
 *       LZ4MI_ERR_RANGE counts nothing here, because it writes nothing (there its bytes are copied clipped at the
 *       content size and counted up to it);
 *   [7] may have become OUT_CAP, LAYOUT, DEPENDENT (never with LZ4MI_FRAMES_CHAINS), HASH_4G, UNSIZED_EXACT (LZ4MI_JS_EXACT given to this call
 *       only: a frame without a content size is declined here as the index call would have) or CAP_BLOCKS (finfo
 *       does not fit nblocks).
 * A frame with status 0 and a content size holds content-size bytes, zeros behind what its blocks wrote (the
 * reference's zero-initialised result). Every block is decoded isolated: no frame reads or writes another
 * frame's bytes, a lone block included.
 * LZ4MI_FRAMES_CHAINS: behind the isolated launch one wave per frame decodes, in block order, (a) every block of a
 * frame with FLG without 0x20 and more than one block (the isolated launch passes these frames over), and (b) of
 * any other frame the blocks from its first one with LZ4MI_ERR_CROSS_BLOCK on -- with LZ4MI_JS_EXACT an
 * independent frame whose tail rewrite reads below a block, a frame flagged independent that is not, block 0
 * reaching below the frame; the blocks before it are final. Each of these blocks is decoded as a lone block (the
 * contract of LZ4MI_LINKED / LZ4MI_LINKED_EXACT: successive one-block calls in index order) of an array that begins
 * at the frame's slot, like the reference's result: a back-reference below the frame's first byte is
 * LZ4MI_ERR_DICT_OOB, and the reference's tail rewrite below position 0 is not written and reads 0 -- no byte of
 * another frame or of the caller's below the slot is read or written. After the first failing block of a frame
 * that block keeps its status and the chain writes nothing of the later ones (LZ4MI_LINKED's after-failure rule,
 * per frame); [0] is that block's error, only the blocks up to and including it decide a decline, [3] counts the
 * blocks with status 0 as without the flag, and such a frame is never declined as DEPENDENT. Every other decline
 * and LZ4MI_VERIFY_CONTENT keep their meaning. Footprint: as below. Cost: a frame's chain is one wave from its
 * first chained block to its last, so the longest frame is the call's floor (the blocks of a 16 MiB frame are
 * walked by one wave): the flag pays with many frames, not with a few long ones. Without the flag the call is
 * what it was, launch for launch.
 * flags: LZ4MI_DEVICE_PTRS | LZ4MI_JS_EXACT (the reference decoder's bytes) | LZ4MI_VERIFY_CONTENT |
 * LZ4MI_FRAMES_CHAINS. Any other
 * flag or a NULL required pointer: LZ4MI_ERR_ARG before the device is looked at; with LZ4MI_FRAMES_CHAINS also a
 * finfo or `out` that is `in`, one of the lists, frame_out_off, frame_out_cap or the other of the two (the call
 * reads those while it writes these). LZ4MI_LINKED* and
 * LZ4MI_VERIFY_BLOCKS are not taken: a linked pass has no barrier at a frame's first slot, and the verify kernel
 * takes a single in_total; block checksums are skipped (lz4mi_frames_verify_blocks, below, checks them between the
 * two calls, with bounds per frame), and without LZ4MI_FRAMES_CHAINS frames with blocks that
 * read the blocks before them are declined (DEPENDENT).
 * A block ends where its size word says: the bytes behind it read as 0, in the index call's measuring and in the
 * decode (the rule of lz4mi_decoded_sizes and lz4mi_decompress_blocks), with or without LZ4MI_FRAMES_CHAINS. The
 * reference reads on in the frame: a cut block whose last offset or length field runs past its end is decoded there
 * with the bytes that follow it (the next size word), here with zeros in their place. Such a frame is not declined
 * and its status is the blocks' (0 where the reference has 0), but its bytes and measured sizes may differ from the
 * reference's; they are equal where the bytes behind the block are 0, as before the EndMark. The caller who must
 * have the reference's bytes for damaged frames asks lz4mi_host_block_read_end per block (a result above the
 * block's end) and decodes such a frame alone, as lz4mi.frame.decompress_frame_device does through its host route.
 * Footprint: finfo; of `out`, only bytes inside out[frame_out_off[f] .. +finfo[f][3]) of frames that were
 * decoded, failed in a block, or were declined as LAYOUT / DEPENDENT (whose bytes there are unspecified). A
 * frame in error or declined before the decode (every other code) has no byte of `out` written. `in` and the
 * lists are read only; the per-block scratch lives with the stream.
 */
int32_t lz4mi_frames_index(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len, uint32_t nframes,
                           uint64_t* blk_in_off, uint32_t* blk_word, uint32_t* blk_frame, uint32_t* blk_size,
                           uint32_t cap_blocks, int64_t* finfo /* nframes x 8 */, int64_t* totals /* 4 */,
                           uint32_t flags, void* stream);
int32_t lz4mi_frames_decompress(const uint8_t* in, const uint64_t* blk_in_off, const uint32_t* blk_word,
                                const uint32_t* blk_frame, const uint32_t* blk_size, uint32_t nblocks,
                                int64_t* finfo, uint32_t nframes, uint8_t* out, const uint64_t* frame_out_off,
                                const uint64_t* frame_out_cap, uint32_t flags, void* stream);
/*
 * lz4mi_frames_verify_blocks: the optional third call, between index and decompress -- the block checksums (FLG
 * 0x10) of every frame of the batch checked on the device, one quad of lanes per record as in lz4mi_verify_blocks,
 * with bounds per frame. Device pointers only (flags must be exactly LZ4MI_DEVICE_PTRS), asynchronous on `stream`,
 * no scratch, nothing read back. It takes the lists and finfo as lz4mi_frames_index left them (nblocks = cap_blocks
 * or totals[1]; totals is not passed and stays the index call's).
 * Frame f is checked when finfo[f][0] == 0, finfo[f][1] & 0x10, it has blocks in the lists (no decline CAP_BLOCKS /
 * PAST_END / EMPTY) and [4] + [6] <= nblocks. Every other decline is irrelevant: a frame declined as MEASURE,
 * SIZE_MISMATCH or UNSIZED_EXACT has its blocks listed and is checked.
 * For block b of a checked frame, b in [finfo[f][4], +finfo[f][6]) with blk_frame[b] == f, the record is the payload
 * in[blk_in_off[b] .. +n), n = blk_word[b] & 0x7FFFFFFF (a stored block's raw bytes are a payload like any other),
 * and the LE32 behind it: blk_status[b] = 0 when that word equals XXH32 (spec convergence, seed 0) of the payload,
 * else LZ4MI_ERR_BLOCK_CHECKSUM. Nothing outside the frame's own range in[frame_off[f] .. +frame_len[f]) is read: a
 * record with blk_in_off[b] < frame_off[f] or blk_in_off[b] + n + 4 > frame_off[f] + frame_len[f] (in 64-bit
 * differences that cannot wrap) is LZ4MI_ERR_BLOCK_CHECKSUM without a byte of it being read -- whatever follows
 * the frame in `in`. Every other entry of blk_status[0 .. nblocks) is set to 0: the blocks of frames that are not
 * checked, a blk_frame[b] >= nframes, an entry that is in no checked frame's range.
 * A checked frame with at least one failing record gets finfo[f][0] = LZ4MI_ERR_BLOCK_CHECKSUM, folded from
 * blk_status by a second pass (one wave per frame), so the outcome does not depend on the order in which records
 * finish, and a frame whose [0] was non-zero keeps its value. Nothing else of finfo changes.
 * lz4mi_frames_decompress then passes such a frame over, as any frame in error, and writes no byte of `out` for it.
 * That is lz4mi_frame_decompress's rule under LZ4MI_VERIFY_BLOCKS: header errors first (the index sets them, and
 * such a frame is not checked), then any failing block checksum before every block's own error (a stored block's
 * LZ4MI_ERR_RANGE included) and before the content checksum.
 * Any flag but LZ4MI_DEVICE_PTRS, a NULL finfo / frame_off / frame_len with nframes > 0, a NULL in / list /
 * blk_status with nblocks > 0, or a finfo or blk_status that is `in`, frame_off, frame_len, one of the lists or
 * the other of the two: LZ4MI_ERR_ARG before the device is looked at. nblocks == 0 or nframes == 0: LZ4MI_OK,
 * nothing is written.
 * Footprint: blk_status[0 .. nblocks) and finfo[f][0] of the frames that fail; nothing else.
 * lz4mi_host_frames_verify_blocks: the same contract on the calling thread (host pointers, no device needed, flags
 * must be 0): the checker of the device pass.
 */
int32_t lz4mi_frames_verify_blocks(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                   uint32_t nframes, const uint64_t* blk_in_off, const uint32_t* blk_word,
                                   const uint32_t* blk_frame, uint32_t nblocks, int64_t* finfo /* nframes x 8 */,
                                   int32_t* blk_status /* nblocks */, uint32_t flags, void* stream);
int32_t lz4mi_host_frames_verify_blocks(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                        uint32_t nframes, const uint64_t* blk_in_off, const uint32_t* blk_word,
                                        const uint32_t* blk_frame, uint32_t nblocks, int64_t* finfo,
                                        int32_t* blk_status, uint32_t flags);
/*
 * lz4mi_frames_index on the calling thread (host pointers, no device needed; flags: LZ4MI_FRAMES_MEASURE |
 * LZ4MI_JS_EXACT): the checker of the device passes. Measuring is lz4mi_host_decoded_size over each block alone.
 */
int32_t lz4mi_host_frames_index(const uint8_t* in, const uint64_t* frame_off, const uint64_t* frame_len,
                                uint32_t nframes, uint64_t* blk_in_off, uint32_t* blk_word, uint32_t* blk_frame,
                                uint32_t* blk_size, uint32_t cap_blocks, int64_t* finfo, int64_t* totals,
                                uint32_t flags);
/*
 * lz4mi_frame_index on the calling thread (host pointers, no device needed): the checker of the single-frame
 * walk, the same function the kernel's lane runs. info as lz4mi_frame_index's.
 */
int32_t lz4mi_host_frame_index(const uint8_t* frame, uint64_t len, uint64_t* pay_off, uint32_t* size_word,
                               uint32_t cap_blocks, int64_t* info);

/*
 * A BATCH OF BUFFERS compressed into one LZ4 frame each on the device: plan, then compress. Device pointers only
 * (LZ4MI_DEVICE_PTRS required), asynchronous on `stream`, nothing is read back by either call.
 * Replaces compressBuffer (src/buffer/bufferCompress.js:100-256) called once per buffer with dictionary = null:
 * frame f is LZ4.compress(in[src_off[f] .. +src_len[f]), null, block_max, true, contentChecksum, addContentSize),
 * byte for byte (any alignment; nothing outside these ranges is read). block_max is resolved as getBlockId does
 * (:77-82): 0 or <= 65536 gives 64 KiB, <= 262144 256 KiB, <= 1048576 1 MiB, anything else 4 MiB.
 * flags (both calls take the same ones): LZ4MI_DEVICE_PTRS | LZ4MI_FRAMES_CONTENT_CHECKSUM (FLG 0x04; one XXH32
 * chain per frame, all frames hashed in one launch that stores the digests in place; a source of 4 GiB or more is
 * declined, LZ4MI_FRAMES_DECLINE_HASH_4G) | LZ4MI_FRAMES_NO_CONTENT_SIZE | LZ4MI_BLOCK_CHECKSUM (FLG 0x10: every
 * record ends with the spec XXH32 of its payload, as in lz4mi_frame_pack; the reference never writes it) |
 * LZ4MI_FRAMES_DEPENDENT (FLG without 0x20, what LZ4.compress(buf) writes by default: a frame of at most one block
 * differs from its independent twin in FLG and the header checksum byte only and is written; one with more blocks
 * is declined, LZ4MI_FRAMES_DECLINE_DEPENDENT: its chain is lz4mi_compress_chain's job) | LZ4MI_FRAMES_PACKED |
 * LZ4MI_FRAMES_CHAINS (only with LZ4MI_FRAMES_DEPENDENT, else LZ4MI_ERR_ARG: an independent FLG over chained blocks
 * would be a broken frame). With it a dependent frame of more than one block is listed by the plan and written by
 * the compress call: its blocks are encoded in order with one hash table carried across them (zeros at the first
 * block, positions relative to the frame's first byte: compressBlock of bufferCompress.js:182-239 with
 * blockIndependence = false), the stored-block rule is applied per block afterwards (a stored block has still
 * updated the table and its raw bytes are history for the next block), and the frame is LZ4.compress(buf, null,
 * block_max, false, contentChecksum, addContentSize) byte for byte. One workgroup walks each such frame
 * (lz4mi_compress_chains_kernel, all frames in one launch); frames of at most one block go through the batch
 * encoder as without the flag. A multi-block source of 0x7FFFFFFF bytes or more stays declined as DEPENDENT (the
 * chain's positions are int32, table values position + 1). Each call reads its own flags: a plan made with the flag
 * and a compress call without it declines these frames as DEPENDENT, and a frame the plan declined stays declined.
 * Any other flag, a NULL required pointer, NULL lists with cap_blocks (nblocks) > 0 or a `work` of less than 16
 * bytes with nblocks > 0: LZ4MI_ERR_ARG before the device is looked at.
 * Out of scope: dictionaries (the reference's prewarm reaches block 0 only; the DictID field is never written),
 * multi-block dependent frames without LZ4MI_FRAMES_CHAINS or of 0x7FFFFFFF bytes or more, splitting one chain over
 * several workgroups (the longest chain of a batch is the call's floor), a spec-variant content checksum, the
 * N-API / JS layer.
 *
 * lz4mi_frames_plan is arithmetic on the lengths (a count, a scan, a fill; one lane per frame). It lists every
 * frame's blocks in frame order, frame after frame: blk_in_off[b] (absolute in `in`), blk_len[b] = min(block_max,
 * rest), blk_frame[b], and blk_work_off[b], the block's slot in `work`: slots are lz4mi_compress_bound(blk_len[b])
 * rounded up to 16 bytes, assigned by an exclusive scan from work[16] on (work[0 .. 16) is where the encoder's
 * waves of blocks that are not encoded put their one byte), so scratch grows with the data, not with
 * nblocks x bound(block_max). finfo[f] (8 x int64 per frame):
 *   [0] 0; [1] FLG | BD << 8; [2] the source length; [3] lz4mi_frame_bound(src_len[f], block_max) after the plan,
 *   the frame's real length after the compress call; [4] its first block in the lists; [5] 0 after the plan, the
 *   frame's position in `out` after the compress call; [6] its block count; [7] 0 = the compress call writes the
 *   frame, else LZ4MI_FRAMES_DECLINE_DEPENDENT / _HASH_4G (neither lists blocks) / _CAP_BLOCKS.
 * A source of length 0 has no blocks and is not declined: the reference writes header, EndMark and, if asked, the
 * checksum of nothing, and so does the compress call. The blocks of the frames that fit are listed without gaps,
 * and a frame whose blocks do not fit cap_blocks lists none. totals (4 x int64): [0] the blocks needed (call again
 * with that cap_blocks if it is above cap_blocks), [1] the blocks listed, [2] the bytes of `out` that suffice in
 * packed mode (the sum of [3] over the frames not declined), [3] the bytes of `work` needed for [0] blocks.
 * Footprint: finfo[0 .. 8 nframes), totals[0 .. 4), and entries [0, totals[1]) of the four lists; nothing else.
 *
 * lz4mi_frames_compress takes the lists and finfo as the plan left them (nblocks = cap_blocks or totals[1]) and,
 * on the one stream: encodes the listed blocks of the frames it will write into `work` with the batch encoder
 * (lz4mi_compress_blocks' kernel, in slices of at most 4096 blocks: 256 MiB of table scratch per stream), and with
 * LZ4MI_FRAMES_CHAINS the blocks of the multi-block dependent frames with one chain per frame instead; sums
 * each frame's record sizes with the reference's stored-block rule (0 < comp < raw, else stored) into finfo[f][3];
 * places the frames; writes every header (its checksum byte included), record position, EndMark and checksum
 * position, one lane per frame; moves every payload once, one wave per block; and fills in the block and content
 * checksums with the batched XXH32.
 * Placing: without LZ4MI_FRAMES_PACKED frame f goes to out[frame_out_off[f] ..) and is declined as
 * LZ4MI_FRAMES_DECLINE_OUT_CAP when it is longer than frame_out_cap[f] or would end behind out_total. With
 * LZ4MI_FRAMES_PACKED (frame_out_off / frame_out_cap may be NULL) the frames that are written lie back to back
 * from out[0] in frame order (a carried device scan of their lengths); a frame that would end behind out_total is
 * declined as OUT_CAP and takes no room. Either way finfo[f][5] is the frame's position.
 * Also declined here, where only the device sees it: a frame whose finfo does not fit nblocks, or one of whose
 * blocks has a slot that is not inside work[16 .. work_bytes) (LZ4MI_FRAMES_DECLINE_CAP_BLOCKS); DEPENDENT and
 * HASH_4G as in the plan, from this call's flags, which also give FLG.
 * Footprint: finfo; of `out`, only out[finfo[f][5] .. +finfo[f][3]) of the frames that are written (finfo[f][7]
 * == 0): a declined frame has no byte of `out` written. `work` is scratch; `in` and the lists are read only.
 */
/* 23 + n + 8 * blocks(n, block_max), block_max resolved as above: header without DictID (15), EndMark, content
 * checksum, and per block a size word and a block checksum around at most n payload bytes (a block that does not
 * shrink is stored). No frame of either call is longer. (An exported function like every other name here: no
 * device needed.) */
uint64_t lz4mi_frame_bound(uint64_t n, uint32_t block_max);
int32_t lz4mi_frames_plan(const uint64_t* src_off, const uint64_t* src_len, uint32_t nframes, uint32_t block_max,
                          uint64_t* blk_in_off, uint32_t* blk_len, uint32_t* blk_frame, uint64_t* blk_work_off,
                          uint32_t cap_blocks, int64_t* finfo /* nframes x 8 */, int64_t* totals /* 4 */,
                          uint32_t flags, void* stream);
int32_t lz4mi_frames_compress(const uint8_t* in, const uint64_t* blk_in_off, const uint32_t* blk_len,
                              const uint32_t* blk_frame, const uint64_t* blk_work_off, uint32_t nblocks,
                              int64_t* finfo, uint32_t nframes, uint8_t* work, uint64_t work_bytes,
                              uint8_t* out, uint64_t out_total, const uint64_t* frame_out_off,
                              const uint64_t* frame_out_cap, uint32_t flags, void* stream);
/*
 * The same two contracts on the calling thread (host pointers, no device needed; flags without
 * LZ4MI_DEVICE_PTRS): the checker of the device passes. The encoder is lz4mi_host_compress_block with a fresh
 * table per block, or with LZ4MI_FRAMES_CHAINS one table carried across a multi-block dependent frame. A `work` that does not hold the slots of the caller's own lists is LZ4MI_ERR_ARG here (the
 * host sees the lists).
 */
int32_t lz4mi_host_frames_plan(const uint64_t* src_off, const uint64_t* src_len, uint32_t nframes, uint32_t block_max,
                               uint64_t* blk_in_off, uint32_t* blk_len, uint32_t* blk_frame, uint64_t* blk_work_off,
                               uint32_t cap_blocks, int64_t* finfo, int64_t* totals, uint32_t flags);
int32_t lz4mi_host_frames_compress(const uint8_t* in, const uint64_t* blk_in_off, const uint32_t* blk_len,
                                   const uint32_t* blk_frame, const uint64_t* blk_work_off, uint32_t nblocks,
                                   int64_t* finfo, uint32_t nframes, uint8_t* work, uint64_t work_bytes,
                                   uint8_t* out, uint64_t out_total, const uint64_t* frame_out_off,
                                   const uint64_t* frame_out_cap, uint32_t flags);


/*
 * Synthetic input generator (bench/test support, not a reference interface):
 * block b = generator `kind` with seed seed0 + b, block_size bytes each,
 * written to out[b * block_size ..] (device pointer, async on stream).
 * kind: 0 random, 1 repetitive (i % 251), 2 tiles216.
 */
int32_t lz4mi_generate_blocks(uint8_t* out, uint32_t kind, uint32_t seed0, uint32_t block_size,
                              uint32_t nblocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LZ4MI_H */
