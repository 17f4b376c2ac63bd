// developer check: the restated glibc pow (as in k_adv.hip gpow15) against libm pow.  gcc -O2 -mfma -ffp-contract=off tools/check_glibc_pow_clone.c -lm
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../extpom_amd/csrc/glibc_pow_tables.h"
static const double A[7] = GPOW_A;
static const double LT[128][3] = GPOW_LOGTAB;
static const double C[4] = GEXP_C;
static const uint64_t ET[256] = GEXP_TAB;
static inline uint64_t asu(double x){uint64_t u;memcpy(&u,&x,8);return u;}
static inline double asd(uint64_t u){double x;memcpy(&x,&u,8);return x;}
#define FMA __builtin_fma
// exp_inline's specialcase(): fused for k > 0 like the fast path; for k < 0 scale * tmp is NOT fused (libm forms the product once and adds it twice)
static double specialcase(double tmp, uint64_t sbits, uint64_t ki){
  double scale, y;
  if((ki&0x80000000ULL)==0){ sbits-=1009ULL<<52; scale=asd(sbits); return 0x1p1009*FMA(scale,tmp,scale); }
  sbits+=1022ULL<<52; scale=asd(sbits);
  y=scale+scale*tmp;
  if(fabs(y)<1.0){
    double hi, lo, one=1.0;
    if(y<0.0) one=-1.0;
    lo=scale-y+scale*tmp; hi=one+y; lo=one-hi+y+lo;
    y=(hi+lo)-one;
    if(y==0.0) y=asd(sbits&0x8000000000000000ULL);
  }
  return 0x1p-1022*y;
}
// x any double, y > 0 of ordinary size: pow's entry for zero, subnormal, inf and nan, the fast path of __ieee754_pow_fma instruction
// for instruction, exp_inline's range test and specialcase() where the result leaves the normal range
double gpow(double x, double y){
  uint64_t ix=asu(x);
  if((unsigned)(ix>>52)-1u>=0x7feu){
    if(2*ix-1>=2*0x7ff0000000000000ULL-1) return x*x;
    if(ix>>63) return (x-x)/(x-x);
    ix=asu(x*0x1p52); ix&=0x7fffffffffffffffULL; ix-=52ULL<<52;
  }
  uint64_t tmp=ix-0x3fe6955500000000ULL;
  int i=(tmp>>45)&127; int64_t k=(int64_t)tmp>>52;
  uint64_t iz=ix-(tmp&0xfff0000000000000ULL);
  double z=asd(iz), kd=(double)k;
  double invc=LT[i][0], logc=LT[i][1], logctail=LT[i][2];
  double t1=FMA(kd,GPOW_LN2HI,logc);
  double r=FMA(z,invc,-1.0);
  double ar=r*A[0];
  double lo1=FMA(kd,GPOW_LN2LO,logctail);
  double q1=FMA(r,A[2],A[1]);
  double q2=FMA(r,A[4],A[3]);
  double t2=r+t1;
  double ar2=r*ar;
  double d1=t1-t2;
  double ar3=r*ar2;
  double lo3=FMA(ar,r,-ar2);
  double lo2=d1+r;
  double q3=FMA(r,A[6],A[5]);
  double hi=t2+ar2;
  double d2=t2-hi;
  double q4=FMA(q3,ar2,q2);
  double lo4=d2+ar2;
  double q5=FMA(ar2,q4,q1);
  double s=lo1+lo2; s=s+lo3; s=s+lo4;
  double lo=FMA(ar3,q5,s);
  double yl=hi+lo;
  double tl=(hi-yl)+lo;
  double ehi=y*yl;
  double e2=FMA(yl,y,-ehi);
  double elo=FMA(y,tl,e2);
  // exp_inline(ehi, elo)
  unsigned abstop=(unsigned)(asu(ehi)>>52)&0x7ffu; int special=0;
  if(abstop-0x3c9u>=0x3fu){
    if(abstop-0x3c9u>=0x80000000u) return 1.0+ehi;
    if(abstop>=0x409u) return (asu(ehi)>>63)? 0x1p-767*0x1p-767 : 0x1p769*0x1p769;
    special=1;
  }
  double kd2=FMA(ehi,GEXP_INVLN2N,GEXP_SHIFT);
  uint64_t ki=asu(kd2);
  kd2=kd2-GEXP_SHIFT;
  double rr=FMA(kd2,GEXP_NEGLN2HIN,ehi);
  rr=FMA(kd2,GEXP_NEGLN2LON,rr);
  unsigned idx=2*(ki&127);
  uint64_t sbits=ET[idx+1]+(ki<<45);
  rr=elo+rr;
  double p1=FMA(rr,C[1],C[0]);
  double s1=rr+asd(ET[idx]);
  double r2=rr*rr;
  double p2=FMA(rr,C[3],C[2]);
  double s2=FMA(p1,r2,s1);
  double r4=r2*r2;
  double tm=FMA(p2,r4,s2);
  if(special) return specialcase(tm,sbits,ki);
  double sc=asd(sbits);
  return FMA(tm,sc,sc);
}
int main(){
  srand48(3); long bad=0,n=20000000;
  for(long t=0;t<20000000;t++){
    double x = (t%3==0)? 30.+10.*drand48() : ((t%3==1)? drand48()*50. : exp(40*(drand48()-0.5)));
    double a=pow(x,1.5), b=gpow(x,1.5);
    if(a!=b){ if(bad<5) printf("x=%a glibc=%a clone=%a\n",x,a,b); bad++; }
  }
  // every binade, the subnormals included (2000 mantissas each), and the values pow's entry answers
  for(int e=-1074;e<=1023;e++) for(int t=0;t<2000;t++){
    double x=ldexp(1.0+drand48(),e), a=pow(x,1.5), b=gpow(x,1.5); n++;
    if(asu(a)!=asu(b)){ if(bad<5) printf("x=%a glibc=%a clone=%a\n",x,a,b); bad++; }
  }
  const double sp[]={0.,0x1p-1074,0x1p-1022,1.,0x1p683,1.7976931348623157e308,INFINITY,NAN,-0.,-1.,-INFINITY};
  for(unsigned q=0;q<sizeof sp/sizeof *sp;q++){
    double a=pow(sp[q],1.5), b=gpow(sp[q],1.5); n++;
    if(asu(a)!=asu(b) && !(a!=a && b!=b)){ if(bad<5) printf("x=%a glibc=%a clone=%a\n",sp[q],a,b); bad++; }
  }
  printf("x**1.5: %ld mismatches of %ld\n",bad,n);
  bad=0;
  for(long t=0;t<2000000;t++){ double x=exp(20*(drand48()-0.5)), y=4*(drand48()-0.5); double a=pow(x,y), b=gpow(x,y); if(a!=b) bad++; }
  printf("general x**y: %ld mismatches of 2000000\n",bad);
  return 0;}
