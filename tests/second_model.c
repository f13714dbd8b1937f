/* second_model.c -- a scalar restatement of what ssw_align (the reference's src/ssw.c) reports as score1 / ref_end1 /
 * score2 / ref_end2 (flag 0: the forward pass only).  DESIGN, "Second-best alignment", has the four rules:
 *   1. the read is padded to 16 rows (byte pass) / 8 rows (word pass) with rows that score 0 against every letter, and
 *      maxColumn[c] is the maximum over real AND padding rows, E and F running through them (ssw.c:108, :215, :448);
 *   2. the byte pass counts when score1 + mismatch < 255, otherwise the word pass (ssw.c:283, :317, :806-810);
 *   3. the mask: columns 0 .. max(end - maskLen, 0) - 1, then from min(end + maskLen, refLen) (word) or one further
 *      (byte, ssw.c:334 against :537); strictly greater replaces, nothing found is 0 / 0, maskLen < 15 is 0 / -1;
 *   4. maskLen is the caller's (second_model.py: mask_len_of, ssw_wrap.py:198-201).
 * read / ref: one code per letter, 0..3, 4 = N (scores 0 on either side, ssw_wrap.py:162-167). */
#include <stdint.h>
#include <stdlib.h>

static int imax(int a, int b) { return a > b ? a : b; }

void second_model(const uint8_t* read, int L, const uint8_t* ref, int refLen, int match, int mismatch, int gap_open,
                  int gap_extend, int mask_len, int32_t out[4]) {
    const int P8 = (L + 7) / 8 * 8, P16 = (L + 15) / 16 * 16;
    int* H = calloc((size_t)P16 + 1, sizeof(int));      /* H[i + 1]: row i of the previous column; H[0]: the row above */
    int* E = calloc((size_t)P16 + 1, sizeof(int));
    int* cw = calloc((size_t)refLen + 1, sizeof(int));   /* column maxima of the word pass's rows and of the byte pass's */
    int* cb = calloc((size_t)refLen + 1, sizeof(int));
    int score1 = 0, end1 = -1;
    for (int c = 0; c < refLen; ++c) {
        int diag = 0, F = 0;
        for (int i = 0; i < P16; ++i) {
            const int q = i < L ? read[i] : 4;           /* a padding row scores like N */
            const int s = (q > 3 || ref[c] > 3) ? 0 : q == ref[c] ? match : -mismatch;
            const int h = imax(imax(diag + s, 0), imax(E[i + 1], F));
            diag = H[i + 1];
            H[i + 1] = h;
            E[i + 1] = imax(E[i + 1] - gap_extend, h - gap_open);
            F = imax(F - gap_extend, h - gap_open);
            if (i < P8) cw[c] = imax(cw[c], h);
            cb[c] = imax(cb[c], h);
        }
        if (cw[c] > score1) { score1 = cw[c]; end1 = c; }
    }
    const int byte_pass = score1 + mismatch < 255;
    const int* col = byte_pass ? cb : cw;
    int score2 = 0, end2 = 0;
    const int left = imax(end1 - mask_len, 0);
    const int right = (end1 + mask_len > refLen ? refLen : end1 + mask_len) + (byte_pass ? 1 : 0);
    for (int c = 0; c < left; ++c)
        if (col[c] > score2) { score2 = col[c]; end2 = c; }
    for (int c = imax(right, 0); c < refLen; ++c)
        if (col[c] > score2) { score2 = col[c]; end2 = c; }
    if (mask_len < 15) { score2 = 0; end2 = -1; }
    out[0] = score1; out[1] = end1; out[2] = score2; out[3] = end2;
    free(H); free(E); free(cw); free(cb);
}
