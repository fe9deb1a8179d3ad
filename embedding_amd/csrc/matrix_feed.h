// matrix_feed.h — the host side of the .matrix reader's transport (matrix_read.hip), free of HIP so that tests/native/matrix_parse_harness.cpp builds it with
// g++: the pieces of seq_pieces.h cut into SLABS.  A slab is a run of at most S bytes of one piece.  Where the piece goes on behind it, it is cut behind the
// last separator or '\n' among its last MAT_CUT bytes, so that no value crosses a slab; where those bytes hold neither, the slab goes out whole — MAT_CUT bytes
// of digits, '\r' and other bytes hold an offence of the rule, the device finds it and no slab follows.  The host looks at those last bytes only: no per-line
// and no per-value work.  The slab goes out framed as matrix_parse.h states: the byte before it in front ('\n' when it opens its piece) and the byte behind it
// at its end (0 when the piece ends), so the kernels look one byte each way without knowing of slabs.
#pragma once
#include "matrix_parse.h"
#include "seq_pieces.h"

#define MAT_CUT 32
#define MAT_SLAB_MIN 256
#define MAT_SLAB_MAX ((int64_t)MAT_TILE * MAT_MAX_TILES)           /* 16 MiB, the default */

namespace {

inline int64_t mat_frame_bytes(int64_t S) { return MAT_LEAD + (S + MAT_LANE - 1) / MAT_LANE * MAT_LANE + MAT_LANE + 1; }      // what next() may write

struct MatrixFeeder {
    std::vector<SeqPiece>& pieces;
    int64_t S;
    uint32_t sep;
    size_t k = 0;                     // the piece
    int64_t sent = 0, got = 0;        // bytes of piece k sent, and read
    uint8_t before = '\n';            // the byte in front of the next slab
    uint8_t keep[MAT_CUT + 1];        // bytes read and not sent
    int64_t n_keep = 0;

    // The next slab framed into buf (mat_frame_bytes(S) bytes): *n = 0 when the pieces are through.  An empty piece gives no slab: *piece skips it, and the
    // caller sees the gap.  *base: the slab's offset in its piece; *first / *last: it opens / ends its piece.
    int next(uint8_t* buf, int64_t* n, int32_t* piece, int64_t* base, bool* first, bool* last) {
        *n = 0;
        while (k < pieces.size() && pieces[k].size == 0) k++;
        if (k >= pieces.size()) return DGE_OK;
        const SeqPiece& p = pieces[k];
        uint8_t* text = buf + MAT_LEAD;
        memset(buf, 0, MAT_LEAD);
        text[-1] = before;
        int64_t have = n_keep;
        if (have) memcpy(text, keep, (size_t)have);
        while (have < S + 1 && got < p.size) {                   // S bytes and the one behind them
            int64_t m = 0;
            if (int rc = seq_piece_read(p, got, text + have, S + 1 - have, &m)) return rc;
            got += m; have += m;
        }
        int64_t send = have;
        const bool ends = have <= S;                             // (then got == p.size: the piece ends in this slab)
        if (!ends) {
            send = S;
            for (int64_t i = S - 1; i >= S - MAT_CUT; i--)
                if (text[i] == sep || text[i] == '\n') { send = i + 1; break; }
        }
        n_keep = have - send;
        if (n_keep) memcpy(keep, text + send, (size_t)n_keep);
        memset(text + send + (ends ? 0 : 1), 0, (size_t)(mat_frame_bytes(S) - MAT_LEAD - send - (ends ? 0 : 1)));      // behind the slab: the next byte, then zeros
        *n = send; *piece = (int32_t)k; *base = sent; *first = sent == 0; *last = ends;
        before = text[send - 1];
        sent += send;
        if (ends) { k++; sent = got = 0; before = '\n'; n_keep = 0; }
        return DGE_OK;
    }
};

}  // namespace
