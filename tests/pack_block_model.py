"""What the models of the two pack kernels share (huff_pack_model: k_huff_pack, fe_pack_model:
k_fe_pack), restated from the block body both kernels call (dc_pack_block.inc): the block constants,
the store phase's cuts, and how a planted sequence of blocks reaches one workgroup (TEST
INFRASTRUCTURE: plain arithmetic, no import of the product). The numbers are those of
dc_core.hip, restated by hand: a change there must be made here with it.
"""
BLOCK = 32768               # DC_BLOCK_BYTES
PIECE = 4096                # PACK_TILE: 256 lanes x 16 bytes
PIECES = BLOCK // PIECE
PACK_BLK_WORDS = 9216       # the stage: a full block at 9 bits per symbol exactly
GROUP = 64                  # DC_SYNC_GROUP
PLAN_WG_BLOCKS = 64         # blocks per workgroup of k_block_local / k_block_final_wide


def words_touched(bit_base, bits):
    """words that hold a bit of the stream (dc_huff_words_needed without its slack)"""
    return ((bit_base & 31) + bits + 31) >> 5


def store_cuts(sh, nw_blk, ends_on_word, vec_out):
    """pack_store_block's cuts for a block of nw_blk words staged from stage word sh on: nwa,
    last_plain (plain stores: stage words (sh, last_plain)), last_or (t == 64 ORs the last word), and
    with vec_out the whole uint4s (nq) and the single words before (head) and after them (tail)."""
    nwa = sh + nw_blk
    last_plain = nwa if ends_on_word else nwa - 1
    r = {"nwa": nwa, "last_plain": last_plain, "last_or": last_plain < nwa and nw_blk > 1}
    if vec_out:
        nq = last_plain >> 2
        tb = 4 * nq if nq > 0 else 4
        r.update(nq=nq, head=max(0, min(last_plain, 4) - sh - 1), tail=max(0, last_plain - tb))
    return r


def seq_layout(steps, grid):
    """([(block positions of a run of steps inside one workgroup, those steps)], blocks in all).
    Block 0 is a filler: its sh is 0 by definition. Under grid g a workgroup runs blocks b, b + g,
    b + 2 g ..; by default (a block pair per workgroup, G = blocks / 2 workgroups) it runs b and
    b + G, so a sequence of three reaches it as its two pairs."""
    if grid == 0:
        runs = len(steps) - 1
        return [([2 * j + 1, 2 * j + 1 + 2 * runs], steps[j: j + 2]) for j in range(runs)], 4 * runs
    return [([1 + i * grid for i in range(len(steps))], steps)], (len(steps) - 1) * grid + 2
