"""The prototype the restatement in tests/test_tsdf.py grew from: TSDF fusion and surface nets in numpy fp64 on an analytic sphere.  Where it
and include/dmvs.h differ in a detail (it forms u from K and E separately and carries no colours), the header holds.  Run it to print the
sphere figures the tests quote."""
import numpy as np, itertools, sys
def look_at(c):
    z = -c/np.linalg.norm(c); up = np.array([0.,0.,1.]) if abs(z[2])<0.9 else np.array([0.,1.,0.])
    x = np.cross(up,z); x/=np.linalg.norm(x); y=np.cross(z,x)
    R=np.stack([x,y,z]); E=np.eye(4); E[:3,:3]=R; E[:3,3]=-R@c; return E
def render_sphere(K,E,H,W,Rad):
    ys,xs=np.meshgrid(np.arange(H,dtype=float),np.arange(W,dtype=float),indexing='ij')
    Kinv=np.linalg.inv(K); ray=np.stack([Kinv[i,0]*xs+Kinv[i,1]*ys+Kinv[i,2] for i in range(3)],-1)  # z=1
    c=E[:3,:3]@np.zeros(3)+E[:3,3]  # sphere centre in cam
    a=(ray*ray).sum(-1); b=-2*(ray@c); cc=c@c-Rad*Rad; disc=b*b-4*a*cc
    t=np.where(disc>0,(-b-np.sqrt(np.maximum(disc,0)))/(2*a),0.0)
    return t.astype(np.float32), (disc>0)
def integrate(depth,mask,Ks,Es,origin,h,dims,tau,Q=16384):
    nx,ny,nz=dims; S=np.zeros((nz,ny,nx),np.int64); Wt=np.zeros((nz,ny,nx),np.int64)
    k,j,i=np.meshgrid(np.arange(nz),np.arange(ny),np.arange(nx),indexing='ij')
    X=origin[0]+i*h; Y=origin[1]+j*h; Z=origin[2]+k*h
    for v in range(len(depth)):
        K,E=Ks[v],Es[v]; H,W=depth[v].shape
        q=[((E[r,0]*X+E[r,1]*Y)+E[r,2]*Z)+E[r,3] for r in range(3)]
        with np.errstate(all='ignore'):
            u=((K[0,0]*q[0]+K[0,1]*q[1])+K[0,2]*q[2])/q[2]; w=((K[1,1]*q[1])+K[1,2]*q[2])/q[2]
            ok=(q[2]>0)&np.isfinite(u)&np.isfinite(w)
            pu=np.rint(u); pw=np.rint(w); ok&=(pu>=0)&(pu<=W-1)&(pw>=0)&(pw<=H-1)
            iu=np.where(ok,pu,0).astype(int); iw=np.where(ok,pw,0).astype(int)
            d=depth[v][iw,iu].astype(np.float64); ok&=mask[v][iw,iu]&np.isfinite(d)&(d>0)
            sdf=d-q[2]; ok&=(sdf>=-tau)
            t=np.minimum(sdf/tau,1.0); qn=np.rint(t*Q).astype(np.int64)
        S+=np.where(ok,qn,0); Wt+=ok
    return S,Wt
EDGES=[(a,b) for a in range(8) for b in range(8) if a<b and bin(a^b).count('1')==1]
def extract(S,Wt,origin,h,min_w=1):
    nz,ny,nx=S.shape; obs=Wt>=min_w
    with np.errstate(all='ignore'): f=np.where(obs,S/np.maximum(Wt,1),np.nan)
    cz,cy,cx=nz-1,ny-1,nx-1
    def corner(c): dx,dy,dz=c&1,(c>>1)&1,(c>>2)&1; return (slice(dz,dz+cz),slice(dy,dy+cy),slice(dx,dx+cx))
    F=[f[corner(c)] for c in range(8)]; O=np.all([obs[corner(c)] for c in range(8)],0)
    neg=[Fc<0 for Fc in F]
    acc=np.zeros((cz,cy,cx,3)); n=np.zeros((cz,cy,cx),int)
    for a,b in EDGES:
        cr=O&(neg[a]!=neg[b])
        with np.errstate(all='ignore'): t=F[a]/(F[a]-F[b])
        pa=np.array([a&1,(a>>1)&1,(a>>2)&1],float); pb=np.array([b&1,(b>>1)&1,(b>>2)&1],float)
        p=pa+(pb-pa)*np.where(cr,t,0)[...,None]
        acc+=np.where(cr[...,None],p,0); n+=cr
    has=n>0; idx=-np.ones((cz,cy,cx),int); idx[has]=np.arange(has.sum())
    kk,jj,ii=np.nonzero(has); loc=acc[has]/n[has][:,None]
    verts=np.stack([origin[0]+(ii+loc[:,0])*h,origin[1]+(jj+loc[:,1])*h,origin[2]+(kk+loc[:,2])*h],1).astype(np.float32)
    faces=[]
    fneg=np.where(obs,f<0,False)
    for k in range(nz):
      for j in range(ny):
        for i in range(nx):
          for ax in range(3):
            e=[0,0,0]; e[ax]=1
            i2,j2,k2=i+e[0],j+e[1],k+e[2]
            if i2>=nx or j2>=ny or k2>=nz: continue
            if not(obs[k,j,i] and obs[k2,j2,i2]) or fneg[k,j,i]==fneg[k2,j2,i2]: continue
            b,c=(ax+1)%3,(ax+2)%3
            cells=[]
            for db,dc in ((-1,-1),(0,-1),(0,0),(-1,0)):
                p=[i,j,k]; p[b]+=db; p[c]+=dc
                if min(p)<0 or p[0]>=cx or p[1]>=cy or p[2]>=cz: cells=None;break
                q=idx[p[2],p[1],p[0]]
                if q<0: cells=None;break
                cells.append(q)
            if cells is None: continue
            if not fneg[k,j,i]: cells=cells[::-1]
            faces+= [(cells[0],cells[1],cells[2]),(cells[0],cells[2],cells[3])]
    return verts,np.array(faces)
if __name__=="__main__":
    Rad=1.0; H,W=61,77; K=np.array([[90.,0,38.],[0,88.,30.],[0,0,1]])
    dirs=[np.array(d,float) for d in itertools.product((-1,1),repeat=3)]+[np.array(d,float) for d in ((1,0,0),(-1,0,0),(0,1,0),(0,-1,0),(0,0,1.),(0,0,-1.))]
    Es=[look_at(d/np.linalg.norm(d)*3.2) for d in dirs]; Ks=[K]*len(Es)
    dm=[render_sphere(K,E,H,W,Rad) for E in Es]; depth=[d for d,_ in dm]; mask=[m for _,m in dm]
    print("views",len(Es),"mask frac",np.mean(mask[0]))
    for dims in ((23,21,19),(29,27,25)):
        h=2.7/(min(dims)-1); origin=-0.5*h*(np.array(dims)-1)+np.array([0.013,-0.021,0.008]); tau=4*h
        S,Wt=integrate(depth,mask,Ks,Es,origin,h,dims,tau)
        v,f=extract(S,Wt,origin,h)
        r=np.linalg.norm(v.astype(float),axis=1)
        ed={}
        for t in f:
            for a,b in ((t[0],t[1]),(t[1],t[2]),(t[2],t[0])): ed[(a,b)]=ed.get((a,b),0)+1
        closed=all(ed.get((b,a),0)==1 and n==1 for (a,b),n in ed.items())
        p=v.astype(float); vol=np.einsum('ij,ij->i',p[f[:,0]],np.cross(p[f[:,1]],p[f[:,2]])).sum()/6
        gd=max(np.abs(np.diff(np.where(m,d,np.nan),axis=a))[np.isfinite(np.abs(np.diff(np.where(m,d,np.nan),axis=a)))].max() for d,m in zip(depth,mask) for a in (0,1))
        print(dims,"h",round(h,4),"V",len(v),"F",len(f),"closed",closed,"euler",len(v)-len(ed)//2+len(f),"maxerr/h",np.abs(r-Rad).max()/h,"meanerr/h",np.abs(r-Rad).mean()/h,"vol/true",vol/(4/3*np.pi),"maxgrad/h",gd/h,"unobs frac",np.mean(Wt==0))
