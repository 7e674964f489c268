/* stand-in for htslib/faidx.h: SimplePileupViewer.h only needs the type to exist */
#pragma once
typedef struct faidx_stand_in faidx_t;
